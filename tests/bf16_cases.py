"""Shared by tests/test_bf16_cpu.py and tests/test_gpu_bf16.py: the emulations of the precision='bf16' arithmetic, the switch that puts
one of them in the oracle's place, the problems, the references (computed once per process) and the bars the GPU tests hold the kernel
to — stated here once, so that the CPU suite can hold the fp32-accumulating emulation to the very same bars in the kernel's place.

Nothing under oracle/ is edited: ``oracle.cem_oracle.ensemble_forward`` looks ``gaussian_dist_mlp`` up at call time, so pointing that
module attribute at an emulation for the duration of a ``with emulating(...)`` block makes every oracle function above it
(unfold_sequences, candidate_scores, do_generate_action) run the reduced-precision network."""
import contextlib
import functools

import numpy as np

from ethz_safe_learning_amd import planner
from oracle import cem_oracle as o
from tests import handover_cases as hc
from tests import helpers as hp

F32 = np.float32
SHAPES = [(60, 2, 128), (100, 12, 128), (23, 3, 48)]          # obs, act, units: one / two input blocks per wave, narrow zero-padded layers
SHAPE_IDS = ['obs60', 'obs100', 'obs23_units48']

# ---- the emulations ------------------------------------------------------------------------------------------------------------
emu64 = planner.bf16_reference_forward                        # the contract: bf16 operands, float64 sums


ORDERS = ([1, 3, 0, 2], [3, 2, 1, 0], [2, 0, 3, 1])             # visiting orders of a 128-feature stage's four K = 32 chunks


def emu32(x, w, order=0):
    """The same contract with the DEVICE's kind of sum: float32 accumulation that starts from the bias and takes the k index in
    chunks of 32 in a permuted order (one accumulator update per chunk, as one MFMA makes) — a stand-in for the kernel on the CPU.
    It differs from emu64 the way the kernel may: by the order of float32 sums, and by the rare activation that lands on the other
    side of a bf16 tie because of it.  `order` picks one of ORDERS: three stand-ins whose ties fall differently."""
    dt = np.asarray(x).dtype

    def dense(h, W, b):
        hr, Wr = planner.rn_bf16(h), planner.rn_bf16(W)
        acc = np.broadcast_to(np.asarray(b, F32), (hr.shape[0], Wr.shape[1])).astype(F32)
        chunks = [(k0, min(k0 + 32, Wr.shape[0])) for k0 in range(0, Wr.shape[0], 32)]
        for k0, k1 in sorted(chunks, key=lambda c: ORDERS[order].index((c[0] // 32) % 4)):
            acc = (acc.astype(np.float64) + hr[:, k0:k1].astype(np.float64) @ Wr[k0:k1].astype(np.float64)).astype(F32)
        return acc
    h = np.asarray(x, F32)
    for W, b in zip(w['W'], w['b']):
        h = np.maximum(dense(h, W, b), F32(0))
    mu = dense(h, w['W_mu'], w['b_mu'])
    var = o.softplus_tf(dense(h, w['W_var'], w['b_var'])) + F32(1e-4)
    return mu.astype(dt), var.astype(dt)


@contextlib.contextmanager
def emulating(forward):
    """oracle.cem_oracle.gaussian_dist_mlp = forward inside the block (restored on the way out, whatever happens)"""
    saved = o.gaussian_dist_mlp
    o.gaussian_dist_mlp = forward
    try:
        yield
    finally:
        o.gaussian_dist_mlp = saved


def unfold_with_moments(s0, actions, weights, members, inputs_min, inputs_max, eps_model):
    """oracle.unfold_sequences that also returns the heads' moments: (traj [B, H + 1, O], mu [B, H, O], sd [B, H, O])"""
    dt = s0.dtype
    B, H, _ = actions.shape
    O = s0.shape[1]
    traj, mus, sds = np.empty((B, H + 1, O), dt), np.empty((B, H, O), dt), np.empty((B, H, O), dt)
    s = s0.copy()
    for t in range(H):
        traj[:, t] = s
        x = o.scale(np.concatenate([s, actions[:, t].astype(dt)], axis=1), inputs_min, inputs_max, True)
        mus[:, t], sds[:, t], sample = o.ensemble_call(x, weights, members, eps_model[t])
        s = s + sample
    traj[:, H] = s
    return traj, mus, sds


# ---- the bars --------------------------------------------------------------------------------------------------------------------
RATIO = 0.05          # K <= RATIO * M: the kernel differs from the emulation by float32 summation order (1e-7 relative) and the rare
                      # activation on the other side of a bf16 tie (3e-5 of them, one more rounding error each): expected 0.001 - 0.01;
                      # truncation instead of RNE, an unrounded operand, a stale plane or a dropped chunk give a ratio near or above 1
NEAR_CAP = 0.10       # at most this fraction of the candidates may sit within helpers.NEAR of a threshold
ATOL = 5e-6           # the fp32 kernels' score bound (tests/test_gpu_split.py): the floor of the near-threshold candidates' tolerance


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def check_rounding_model(kernel, emu, ref64, what):
    """Per step t (axis 1 of [B, T, O] trajectories; scores: pass [n, 1]): K_t = RMS(kernel - emu) <= RATIO * M_t, M_t = RMS(emu - ref64),
    and max |kernel - emu| <= max |emu - ref64|.  Returns the ratios K_t / M_t (0 where both vanish)."""
    kernel, emu, ref64 = (np.asarray(a, np.float64) for a in (kernel, emu, ref64))
    assert kernel.shape == emu.shape == ref64.shape and np.all(np.isfinite(kernel)), what
    ratios = []
    for t in range(kernel.shape[1]):
        K, M = rms(kernel[:, t] - emu[:, t]), rms(emu[:, t] - ref64[:, t])
        ratios.append(K / M if M > 0 else (0.0 if K == 0 else np.inf))
        assert K <= RATIO * M, '%s step %d: RMS(kernel - emulation) %.3e > %.2f x RMS(emulation - fp64) %.3e' % (what, t, K, RATIO, M)
        mk, mm = np.abs(kernel[:, t] - emu[:, t]).max(), np.abs(emu[:, t] - ref64[:, t]).max()
        assert mk <= mm, '%s step %d: max |kernel - emulation| %.3e > max |emulation - fp64| %.3e' % (what, t, mk, mm)
    return ratios


def check_scores(scores, ref, what):
    """GPU test 3's conditions on one iteration's per-candidate scores.  ref: score_reference(...).  Candidates within helpers.NEAR
    of a threshold (on the emulation's trajectories) must equal one of the admissible outcomes, as helpers.assert_scores_match_oracle
    asks, and are at most NEAR_CAP of all; the rest meet check_rounding_model.  Returns (ratio, near fraction).
    A near-threshold candidate is as exposed to a bf16 tie that falls the other way as a clear one (about one activation per candidate
    does, and moves the score by 1e-5 .. 1e-4), so its distance to the nearest admissible outcome gets the bound the clear candidates'
    distance to the emulation has — the max condition, max |emulation - fp64 oracle| over the clear candidates, a figure of the
    references alone — and never less than the fp32 kernels' ATOL."""
    near = ref['near']
    assert near.mean() <= NEAR_CAP, '%s: %.1f %% of the candidates sit on a threshold' % (what, 100 * near.mean())
    tol = max(ATOL, float(np.abs(ref['emu'][~near].astype(np.float64) - ref['ref64'][~near]).max()))
    best = np.min(np.stack([np.abs(scores - r) / (tol + 6e-8 * np.abs(r)) for r in ref['admissible']]), axis=0)
    bad = np.nonzero(near & (best > 1.0))[0]
    assert bad.size == 0, '%s: %d near-threshold candidates equal none of the admissible outcomes, e.g. %d: %.9g vs nominal %.9g' % (
        what, bad.size, bad[0], scores[bad[0]], ref['emu'][bad[0]])
    c = ~near
    r = check_rounding_model(scores[c][:, None], ref['emu'][c][:, None], ref['ref64'][c][:, None], what)
    return r[0], float(near.mean())


# ---- problems and references ----------------------------------------------------------------------------------------------------
def bf16_config(O, A, U, L=4, E=2, **kw):
    base = dict(obs_dim=O, act_dim=A, units=U, n_layers=L, ensemble_size=E, particles=E, n_samples=32, horizon=3, n_elite=4, iterations=2,
                precision='bf16')
    base.update(kw)
    return hc.config(base)


def image_bf16(cfg, w):
    """uint32 words of one member's precision='bf16' image, restated from the layout: the split stream's units (K = 32 chunk, output
    block) in its visiting order, each [lane(64)][s(8)] bf16 — lane 16 q + i, slot s = RN(W[16 (2 kb + s / 4) + 4 q + s % 4][16 ob + i]),
    zero outside the matrix — then 4 KB of zeros (the prefetch slack)."""
    s = np.arange(8)[None, :]
    parts = []
    for name, kb, ob in hc.units_split(cfg):
        v = hc._gather(hc._matrix(w, name), 16 * (2 * kb + (s >> 2)) + 4 * hc.Q + (s & 3), 16 * ob + hc.I16)
        parts.append((planner.rn_bf16(v).view(np.uint32) >> 16).astype(np.uint16).reshape(-1))
    parts.append(np.zeros(2048, np.uint16))
    return np.ascontiguousarray(np.concatenate(parts)).view(np.uint32)


def exact_problem(O, A, U, E=5, L=4, seed=0):
    """A problem on which every dense output is ONE product plus a bias and every float32 sum is exact, so that the kernel must equal
    the emulation bit for bit whatever its summation order: weights are signed powers of two (1/2, 1, 2) times a random selection matrix
    with one nonzero per column (a permutation where the matrix is square), different per layer and member, heads likewise; biases,
    the state and the actions lie on a 2^-6 grid; the normaliser is min 0 / max 1.  What is left to get wrong is the layout: which
    weight meets which activation, the rounding of the operands, the bias rows, the padding."""
    pb = hp.make_problem(O, A, E, L, seed=3, units=U)
    rng = np.random.default_rng(seed)

    def sel(fi, fo):
        W = np.zeros((fi, fo), F32)
        rows = rng.permutation(fi)[:fo] if fi >= fo else np.concatenate([rng.permutation(fi), rng.integers(0, fi, fo - fi)])
        W[rows, np.arange(fo)] = rng.choice([-1.0, 1.0], fo) * rng.choice([0.5, 1.0, 2.0], fo)
        return W

    def grid(n, lim):
        return (rng.integers(-int(lim * 64), int(lim * 64) + 1, n) / 64.0).astype(F32)
    ws = []
    for _ in range(E):
        Ws, bs, fi = [], [], O + A
        for _ in range(L):
            Ws.append(sel(fi, U)); bs.append(grid(U, 0.25)); fi = U
        ws.append(dict(W=Ws, b=bs, W_mu=(sel(U, O) * F32(0.25)).astype(F32), b_mu=grid(O, 0.125), W_var=sel(U, O), b_var=(grid(O, 1.0) - F32(6.0)).astype(F32)))
    pb['weights'] = ws
    pb['inputs_min'] = np.zeros(O + A, F32); pb['inputs_max'] = np.ones(O + A, F32)
    return pb


def exact_inputs(O, A, B=40, H=3, seed=1):
    rng = np.random.default_rng(seed)
    s0 = (rng.integers(-64, 65, (B, O)) / 64.0).astype(F32)
    acts = (rng.integers(-64, 65, (B, H, A)) / 64.0).astype(F32)
    return s0, acts, np.zeros((H, B, O), F32)


def members_of(B, E):
    return np.arange(B) // (B // E)


@functools.lru_cache(maxsize=None)
def traj_case(dims, B=80, H=8):
    """GPU test 2's problem, inputs and references for one shape: (pb, s0, acts, eps, emulation trajectory, fp64 oracle trajectory)"""
    O, A, U = dims
    pb = hp.make_problem(O, A, 5, 4, seed=7 + O, units=U)
    rng = np.random.default_rng(40 + O)
    s0 = rng.normal(0, 0.3, (B, O)).astype(F32)
    acts = rng.uniform(-1, 1, (B, H, A)).astype(F32)
    eps = rng.standard_normal((H, B, O)).astype(F32)
    args = (s0.astype(np.float64), acts.astype(np.float64), o.cast_weights(pb['weights'], np.float64), members_of(B, 5), pb['inputs_min'], pb['inputs_max'], eps)
    ref64 = o.unfold_sequences(*args)
    with emulating(emu64):
        emu = o.unfold_sequences(*args)
    return pb, s0, acts, eps, emu, ref64


def traj_stand_in(dims, order=0):
    """... and what the fp32-accumulating emulation gives in the kernel's place: float32 state, float32 everything, as on the device"""
    pb, s0, acts, eps, _, _ = traj_case(dims)
    with emulating(functools.partial(emu32, order=order)):
        return o.unfold_sequences(s0, acts, pb['weights'], members_of(s0.shape[0], 5), pb['inputs_min'], pb['inputs_max'], eps)


SCORE_SHAPE = dict(N=256, H=12, P=5, E=5, k=25, I=1)
SCORE_SEED = {60: 21, 100: 21}                                # problem seed = this + obs (chosen on the CPU: tests/test_bf16_cpu.py)


@functools.lru_cache(maxsize=None)
def score_case(O, A, variant):
    """GPU test 3's problem, noise and references: dict(pb, ea, em, ocfg, emu, ref64, near, admissible)"""
    pb = hp.make_problem(O, A, 5, 4, seed=SCORE_SEED[O] + O)
    n = SCORE_SHAPE
    ea, em, _ = hp.noise(n['I'], n['N'], n['H'], A, n['P'], O, seed=5)
    ocfg, _ = hp.configs(pb, variant=variant, post=0.3, **n)
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    actions = o.sample_actions(np.broadcast_to(mu0, (n['H'], A)), np.broadcast_to(sg0, (n['H'], A)), lb, ub, ea[0])
    args = (pb['state'].astype(np.float64), actions.astype(np.float64), o.cast_weights(pb['weights'], np.float64), pb['inputs_min'], pb['inputs_max'],
            em[0], ocfg, pb['scorer'])
    ref64 = o.candidate_scores(*args)
    with emulating(emu64):
        emu, traj = o.candidate_scores(*args, return_traj=True)
    near = o.threshold_margins(traj, pb['scorer']).reshape(n['P'], n['N']).min(axis=0) <= hp.NEAR
    admissible = hp.admissible_scores(traj, n['P'], n['N'], pb['scorer'], variant, 0.3)
    return dict(pb=pb, ea=ea, em=em, ocfg=ocfg, actions=actions, emu=emu, ref64=ref64, near=near, admissible=admissible)


def score_stand_in(O, A, variant, order=0):
    c = score_case(O, A, variant)
    with emulating(functools.partial(emu32, order=order)):
        return o.candidate_scores(c['pb']['state'], c['actions'].astype(F32), c['pb']['weights'], c['pb']['inputs_min'], c['pb']['inputs_max'],
                                  c['em'][0], c['ocfg'], c['pb']['scorer'])


PLAN_SHAPE = dict(N=128, H=8, P=5, E=5, k=12, I=3)
PLAN_SEED = {60: 7, 100: 7, 23: 7}                            # problem seed = this + obs (chosen on the CPU: tests/test_bf16_cpu.py)


@functools.lru_cache(maxsize=None)
def plan_case(dims, variant):
    """GPU test 5's problem, noise and the oracle's plan under the emulation: dict(pb, noise, ocfg, ref = (action, score, iterations))"""
    O, A, U = dims
    pb = hp.make_problem(O, A, 5, 4, seed=PLAN_SEED[O] + O, units=U)
    n = PLAN_SHAPE
    ocfg, _ = hp.configs(pb, variant=variant, noise=0.01, post=0.3, **n)
    ea, em, eo = hp.noise(n['I'], n['N'], n['H'], A, n['P'], O, seed=3)
    with emulating(emu64):
        ref = o.do_generate_action(pb['state'], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'], ea, em, eo, ocfg, pb['scorer'])
    return dict(pb=pb, noise=(ea, em, eo), ocfg=ocfg, ref=ref)


def plan_stand_in(dims, variant, order=0):
    c = plan_case(dims, variant)
    pb, (ea, em, eo) = c['pb'], c['noise']
    with emulating(functools.partial(emu32, order=order)):
        return o.do_generate_action(pb['state'], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'], ea, em, eo, c['ocfg'], pb['scorer'])


def check_plan(got, ref, what):
    """GPU test 5's bars (the split test's): iteration count equal, score within 2e-5, action within 1e-5 relative"""
    (a, s, it), (ra, rs, rit) = got, ref
    assert it == rit and abs(float(s) - float(rs)) <= 2e-5, (what, s, rs, it, rit)
    np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-6, err_msg=what)
