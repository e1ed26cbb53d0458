"""Shared by tests/test_bf16_cpu.py and tests/test_gpu_bf16.py: the emulations of the precision='bf16' arithmetic, the switch that puts
one of them in the oracle's place, the problems, the references (computed once per process) and the bars the GPU tests hold the kernel
to — stated here once, so that the CPU suite can hold the fp32-accumulating emulation to the very same bars in the kernel's place.

Nothing under oracle/ is edited: ``oracle.cem_oracle.ensemble_forward`` looks ``gaussian_dist_mlp`` up at call time, so pointing that
module attribute at an emulation for the duration of a ``with emulating(...)`` block makes every oracle function above it
(unfold_sequences, candidate_scores, do_generate_action) run the reduced-precision network."""
import contextlib
import functools
import itertools

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


_FIRST =([1, 3, 0, 2], [3, 2, 1, 0], [2, 0, 3, 1])              # (orders 0 - 2 are the ones the fixed cases' seeds were chosen under)
ORDERS = _FIRST + tuple(list(p) for p in itertools.permutations(range(4)) if list(p) not in _FIRST)   # all 24 visiting orders of a
                                                                  # 128-feature stage's four K = 32 chunks


FINE = ((1, False), (1, True), (2, False), (2, True))     # (group, descending) of the fine-grained stand-ins: a float32 rounding after
                                                          # every product / every two products, k up / k down


def emu32(x, w, order=0, group=32, descending=False):
    """The same contract with the DEVICE's kind of sum: float32 accumulation that starts from the bias and takes the k index in
    chunks of 32 in a permuted order (one accumulator update per chunk, as one MFMA makes) — a stand-in for the kernel on the CPU.
    It differs from emu64 the way the kernel may: by the order of float32 sums, and by the rare activation that lands on the other
    side of a bf16 tie because of it.  `order` picks one of ORDERS: stand-ins whose ties fall differently (the fixed cases use the first
    three, the seed screening of tests/bf16_fuzz_cases.py all 24).
    `group` < 32 rounds the accumulator after every `group` products instead (k ascending or descending; `order` is then unused): how
    the matrix pipe sums WITHIN an MFMA is not documented, and on the device ties have fallen the way of group = 1 where none of the 24
    chunk orders put them (tests/bf16_fuzz_cases.py DROPPED) — so the screenings run the FINE stand-ins as well."""
    dt = np.asarray(x).dtype

    def dense(h, W, b):
        hr, Wr = planner.rn_bf16(h), planner.rn_bf16(W)
        acc = np.broadcast_to(np.asarray(b, F32), (hr.shape[0], Wr.shape[1])).astype(F32)
        chunks = [(k0, min(k0 + group, Wr.shape[0])) for k0 in range(0, Wr.shape[0], group)]
        chunks = sorted(chunks, key=lambda c: ORDERS[order].index((c[0] // 32) % 4)) if group == 32 else (chunks[::-1] if descending else chunks)
        for k0, k1 in chunks:
            acc = (acc.astype(np.float64) + hr[:, k0:k1].astype(np.float64) @ Wr[k0:k1].astype(np.float64)).astype(F32)
        return acc
    h = np.asarray(x, F32)
    for W, b in zip(w['W'], w['b']):
        h = np.maximum(dense(h, W, b), F32(0))
    mu = dense(h, w['W_mu'], w['b_mu'])
    var = o.softplus_tf(dense(h, w['W_var'], w['b_var'])) + F32(1e-4)
    return mu.astype(dt), var.astype(dt)


def stand_ins():
    """{name: forward} of every stand-in the screenings hold to half the bar: the 24 chunk orders and the FINE ones"""
    out = {'order %d' % i: functools.partial(emu32, order=i) for i in range(len(ORDERS))}
    out.update({'group %d %s' % (g, 'down' if d else 'up'): functools.partial(emu32, group=g, descending=d) for g, d in FINE})
    return out


def trunc_bf16(x):
    """x (as float32) with its low 16 bits cut off: round towards zero, the rounding the contract does NOT ask for"""
    x = np.ascontiguousarray(x, F32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)


MUTANTS = ('trunc_act', 'trunc_w', 'raw_input', 'raw_heads', 'raw_var', 'drop_chunk', 'bias_bf16')
SCORE_BLIND = ('raw_var',)         # scores do not see the variance head's input rounding (its ratios are the stand-ins'): moments must


def mutant(kind):
    """emu64 made wrong in ONE way — a kernel fault the bars must catch (tests/test_bf16_bars_cpu.py puts each in the kernel's place):
    trunc_act   activations truncated to bf16 instead of rounded to nearest even
    trunc_w     weights truncated
    raw_input   the layer-0 input left unrounded
    raw_heads   the input of both heads left unrounded
    raw_var     the input of the variance head alone left unrounded
    drop_chunk  one K = 32 chunk (the second; the only one where there is one) of the second dense stage (the only one of a one-layer
                network) left out of the sum
    bias_bf16   biases rounded to bf16
    Sums are float64, as in emu64: a mutant differs from the contract by its fault alone."""
    assert kind in MUTANTS, kind
    rw = trunc_bf16 if kind == 'trunc_w' else planner.rn_bf16
    ra = trunc_bf16 if kind == 'trunc_act' else planner.rn_bf16
    rb = planner.rn_bf16 if kind == 'bias_bf16' else (lambda b: np.asarray(b, F32))

    def forward(x, w):
        dt = np.asarray(x).dtype

        def dense(h, W, b, raw=False, drop=False):
            hr = (np.asarray(h, F32) if raw else ra(h)).astype(np.float64)
            Wr = rw(W).astype(np.float64)
            if drop:
                k0 = 32 if Wr.shape[0] > 32 else 0
                hr = hr.copy(); hr[:, k0:k0 + 32] = 0.0
            return (hr @ Wr + rb(b).astype(np.float64)).astype(F32)
        h = np.asarray(x, F32)
        n = len(w['W'])
        for i, (W, b) in enumerate(zip(w['W'], w['b'])):
            h = np.maximum(dense(h, W, b, raw=(kind == 'raw_input' and i == 0), drop=(kind == 'drop_chunk' and i == min(1, n - 1))), F32(0))
        mu = dense(h, w['W_mu'], w['b_mu'], raw=kind == 'raw_heads')
        var = o.softplus_tf(dense(h, w['W_var'], w['b_var'], raw=kind in ('raw_heads', 'raw_var'))) + F32(1e-4)
        return mu.astype(dt), var.astype(dt)
    return forward


@contextlib.contextmanager
def emulating(forward):
    """oracle.cem_oracle.gaussian_dist_mlp = forward inside the block (restored on the way out, whatever happens)"""
    saved = o.gaussian_dist_mlp
    o.gaussian_dist_mlp = forward
    try:
        yield
    finally:
        o.gaussian_dist_mlp = saved


def unfold_with_moments(s0, actions, weights, members, inputs_min, inputs_max, eps_model, scale_features=True, sampling_propagation=True):
    """oracle.unfold_sequences that also returns the heads' moments: (traj [B, H + 1, O], mu [B, H, O], sd [B, H, O])"""
    dt = s0.dtype
    B, H, _ = actions.shape
    O = s0.shape[1]
    traj, mus, sds = np.empty((B, H + 1, O), dt), np.empty((B, H, O), dt), np.empty((B, H, O), dt)
    s = s0.copy()
    for t in range(H):
        traj[:, t] = s
        x = o.scale(np.concatenate([s, actions[:, t].astype(dt)], axis=1), inputs_min, inputs_max, scale_features)
        mus[:, t], sds[:, t], sample = o.ensemble_call(x, weights, members, eps_model[t])
        s = s + (sample if sampling_propagation else mus[:, t])
    traj[:, H] = s
    return traj, mus, sds


# ---- the bars --------------------------------------------------------------------------------------------------------------------
RATIO = 0.05          # K <= RATIO * M: the kernel differs from the emulation by float32 summation order (1e-7 relative) and the rare
                      # activation on the other side of a bf16 tie (3e-5 of them, one more rounding error each): the stand-ins give
                      # 0.0001 - 0.045, the device 0.0001 - 0.04.  What the bar catches is what tests/test_bf16_bars_cpu.py and
                      # tests/test_bf16_fuzz_cpu.py show, no more: truncated activations or weights, rounded biases and a dropped chunk
                      # miss it on trajectories (ratio about 3 and up at step 1) and on scores; an unrounded layer-0 or head input misses it
                      # on trajectories and on the QUANTILES of the scores over the flip-free candidates, on every case, but can pass
                      # the scores' RMS condition, whose yardstick threshold flips inflate; an unrounded variance-head input is seen
                      # by sd alone.  A stale LDS plane has no emulation here.
NEAR_CAP = 0.10       # at most this fraction of the candidates may sit within helpers.NEAR of a threshold
Y_MIN = 0.80          # ... and at least this fraction is clear AND resolves every comparison as the fp64 oracle does (a condition on the
                      # references, met on the CPU: 82 - 100 % on every case of the suites)
ATOL = 5e-6           # the fp32 kernels' score bound (tests/test_gpu_split.py): the floor of the near-threshold candidates' tolerance


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, np.float64)))))


def check_rounding_model(kernel, emu, ref64, what, ratio=RATIO):
    """Per step t (axis 1 of [B, T, O] trajectories; scores: pass [n, 1]): K_t = RMS(kernel - emu) <= RATIO * M_t, M_t = RMS(emu - ref64),
    and max |kernel - emu| <= max |emu - ref64|.  Returns the ratios K_t / M_t (0 where both vanish).  `ratio`: the seed screening of
    tests/bf16_fuzz_cases.py holds the stand-ins to RATIO / 2."""
    kernel, emu, ref64 = (np.asarray(a, np.float64) for a in (kernel, emu, ref64))
    assert kernel.shape == emu.shape == ref64.shape and np.all(np.isfinite(kernel)), what
    ratios = []
    for t in range(kernel.shape[1]):
        K, M = rms(kernel[:, t] - emu[:, t]), rms(emu[:, t] - ref64[:, t])
        ratios.append(K / M if M > 0 else (0.0 if K == 0 else np.inf))
        assert K <= ratio * M, '%s step %d: RMS(kernel - emulation) %.3e > %.3f x RMS(emulation - fp64) %.3e' % (what, t, K, ratio, M)
        mk, mm = np.abs(kernel[:, t] - emu[:, t]).max(), np.abs(emu[:, t] - ref64[:, t]).max()
        assert mk <= mm, '%s step %d: max |kernel - emulation| %.3e > max |emulation - fp64| %.3e' % (what, t, mk, mm)
    return ratios


def threshold_outcomes(traj, sp):
    """[B, H + 1, 1 + kinds] bool: how every thresholded comparison of the scorer resolves on a trajectory — goal_achieved
    (goal_distance_metric <= 0.8 goal_size) and, per constrained cost kind, closest_distance <= size: the quantities
    oracle.threshold_margins visits, as outcomes instead of margins."""
    out = []
    for t in range(traj.shape[1]):
        row = [o.goal_distance_metric(traj[:, t], sp).astype(np.float64) <= sp.goal_size * 0.8]
        for lo, hi, size in sp.cost_kinds:
            row.append(o.closest_distance(traj[:, t, lo:hi], sp).astype(np.float64) <= size)
        out.append(np.stack(row, axis=1))
    return np.stack(out, axis=1)


def score_reference(pb, actions, eps_model_it, ocfg):
    """The references of one iteration's scores: dict(emu, ref64: scores under the emulation / the fp64 oracle; traj, traj64: their
    trajectories; near: candidates with a comparison within helpers.NEAR of its threshold on the emulation's trajectory; admissible:
    helpers.admissible_scores there; flip_free: candidates all of whose P rows resolve EVERY comparison alike on the two trajectories)"""
    P, n = ocfg.particles, actions.shape[0]
    args = (pb['state'].astype(np.float64), actions.astype(np.float64), o.cast_weights(pb['weights'], np.float64), pb['inputs_min'], pb['inputs_max'],
            eps_model_it, ocfg, pb['scorer'])
    ref64, traj64 = o.candidate_scores(*args, return_traj=True)
    with emulating(emu64):
        emu, traj = o.candidate_scores(*args, return_traj=True)
    near = o.threshold_margins(traj, pb['scorer']).reshape(P, n).min(axis=0) <= hp.NEAR
    admissible = hp.admissible_scores(traj, P, n, pb['scorer'], ocfg.variant, ocfg.posterior_mean_threashold)
    same = threshold_outcomes(traj, pb['scorer']) == threshold_outcomes(traj64, pb['scorer'])
    return dict(emu=emu, ref64=ref64, traj=traj, traj64=traj64, near=near, admissible=admissible, flip_free=same.reshape(P, n, -1).all(axis=(0, 2)))


def flip_free_set(ref):
    """Y: the clear candidates whose comparisons resolve alike under the emulation and the fp64 oracle"""
    return ~ref['near'] & ref['flip_free']


def score_figures(scores, ref):
    """The figures check_scores compares, as text and without asserting (printed before the assertion, so a failure shows them all)"""
    c, Y = ~ref['near'], flip_free_set(ref)
    dk, dm = np.abs(np.asarray(scores, np.float64) - ref['emu']), np.abs(ref['emu'].astype(np.float64) - ref['ref64'])
    if not Y.any() or not c.any():
        return 'no clear candidates'
    return 'clear %d of %d: RMS %.3e vs %.3e, max %.3e vs %.3e | flip-free %d: median %.3e vs %.3e, 90th percentile %.3e vs %.3e, RMS %.3e vs %.3e' % (
        c.sum(), c.size, rms(dk[c]), rms(dm[c]), dk[c].max(), dm[c].max(), Y.sum(), np.median(dk[Y]), np.median(dm[Y]),
        np.percentile(dk[Y], 90), np.percentile(dm[Y], 90), rms(dk[Y]), rms(dm[Y]))


def check_scores(scores, ref, what, ratio=RATIO):
    """GPU test 3's conditions on one iteration's per-candidate scores.  ref: score_reference(...).  Candidates within helpers.NEAR
    of a threshold (on the emulation's trajectories) must equal one of the admissible outcomes, as helpers.assert_scores_match_oracle
    asks, and are at most NEAR_CAP of all; the rest meet check_rounding_model.
    A near-threshold candidate is as exposed to a bf16 tie that falls the other way as a clear one (about one activation per candidate
    does, and moves the score by 1e-5 .. 1e-4), so its distance to the nearest admissible outcome gets the bound the clear candidates'
    distance to the emulation has — the max condition, max |emulation - fp64 oracle| over the clear candidates, a figure of the
    references alone — and never less than the fp32 kernels' ATOL.
    That yardstick — RMS and max of emulation - fp64 over the clear candidates — is inflated by the few candidates that the bf16
    rounding itself (1e-4 .. 1e-3 per state) puts on the other side of a threshold: they differ from the oracle by the goal reward or
    the 100 of the safe penalty, and lift the RMS 2 to 10 000 times over the rounding's own size.  So, over Y = the clear candidates
    whose every comparison resolves alike on the two references' trajectories (at least Y_MIN of all), two more conditions:
    median |kernel - emulation| <= RATIO x median |emulation - fp64| and the same at the 90th percentile.  (Quantiles, not an RMS over Y:
    ONE candidate whose score a bf16 tie moved lifts the stand-ins' RMS ratio over Y to 0.04.)
    Returns (RMS ratio over the clear candidates, near fraction, median ratio over Y, 90th-percentile ratio over Y)."""
    bars, figures = _score_bars(scores, ref, what, ratio)
    for _, ok, message in bars:
        assert ok, message
    return figures


def failed_score_bars(scores, ref, ratio=RATIO):
    """Which of check_scores' bars on the KERNEL a score vector misses, all of them and not only the first: a subset of
    ('near', 'rms', 'max', 'median', 'p90').  (The conditions on the references alone — NEAR_CAP, Y_MIN — are asserted.)"""
    return tuple(tag for tag, ok, _ in _score_bars(scores, ref, '', ratio)[0] if not ok)


def _score_bars(scores, ref, what, ratio):
    near = ref['near']
    assert near.mean() <= NEAR_CAP, '%s: %.1f %% of the candidates sit on a threshold' % (what, 100 * near.mean())
    Y = flip_free_set(ref)
    assert Y.mean() >= Y_MIN, '%s: only %.1f %% of the candidates are clear of every threshold under both references' % (what, 100 * Y.mean())
    scores = np.asarray(scores)
    assert scores.shape == ref['emu'].shape and np.all(np.isfinite(scores)), what
    dk, dm = np.abs(scores.astype(np.float64) - ref['emu']), np.abs(ref['emu'].astype(np.float64) - ref['ref64'])
    c = ~near
    tol = max(ATOL, float(dm[c].max()))
    best = np.min(np.stack([np.abs(scores - r) / (tol + 6e-8 * np.abs(r)) for r in ref['admissible']]), axis=0)
    bad = np.nonzero(near & (best > 1.0))[0]
    bars = [('near', bad.size == 0, '%s: %d near-threshold candidates equal none of the admissible outcomes, e.g. %s' % (
        what, bad.size, ['%d: %.9g vs nominal %.9g' % (i, scores[i], ref['emu'][i]) for i in bad[:1]]))]
    K, M = rms(dk[c]), rms(dm[c])
    bars.append(('rms', K <= ratio * M, '%s: RMS(kernel - emulation) %.3e > %.3f x RMS(emulation - fp64) %.3e over the clear candidates' % (what, K, ratio, M)))
    bars.append(('max', dk[c].max() <= dm[c].max(), '%s: max |kernel - emulation| %.3e > max |emulation - fp64| %.3e over the clear candidates' % (
        what, dk[c].max(), dm[c].max())))
    q = []
    for pct, tag, name in ((50, 'median', 'median'), (90, 'p90', '90th percentile')):
        k, m = float(np.percentile(dk[Y], pct)), float(np.percentile(dm[Y], pct))
        q.append(k / m if m > 0 else (0.0 if k == 0 else np.inf))
        bars.append((tag, k <= ratio * m, '%s: %s of |kernel - emulation| over the flip-free candidates %.3e > %.3f x that of |emulation - fp64| %.3e' % (
            what, name, k, ratio, m)))
    return bars, ((K / M if M > 0 else (0.0 if K == 0 else np.inf)), float(near.mean()), q[0], q[1])


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
    return traj_under(dims, functools.partial(emu32, order=order))


def traj_under(dims, forward):
    pb, s0, acts, eps, _, _ = traj_case(dims)
    with emulating(forward):
        return o.unfold_sequences(s0, acts, pb['weights'], members_of(s0.shape[0], 5), pb['inputs_min'], pb['inputs_max'], eps)


SCORE_SHAPE = dict(N=256, H=12, P=5, E=5, k=25, I=1)
SCORE_SEED = {60: 21, 100: 21}                                # problem seed = this + obs (chosen on the CPU: tests/test_bf16_cpu.py)


@functools.lru_cache(maxsize=None)
def score_case(O, A, variant):
    """GPU test 3's problem, noise and references: dict(pb, ea, em, ocfg, actions, + score_reference's)"""
    pb = hp.make_problem(O, A, 5, 4, seed=SCORE_SEED[O] + O)
    n = SCORE_SHAPE
    ea, em, _ = hp.noise(n['I'], n['N'], n['H'], A, n['P'], O, seed=5)
    ocfg, _ = hp.configs(pb, variant=variant, post=0.3, **n)
    return _score_case(pb, ea, em, ocfg)


def _score_case(pb, ea, em, ocfg):
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    H, A = ocfg.horizon, pb['low'].shape[0]
    actions = o.sample_actions(np.broadcast_to(mu0, (H, A)), np.broadcast_to(sg0, (H, A)), lb, ub, ea[0])
    return dict(pb=pb, ea=ea, em=em, ocfg=ocfg, actions=actions, **score_reference(pb, actions, em[0], ocfg))


def scores_under(c, forward):
    """what `forward` gives in the kernel's place on a score case: float32 state, float32 everything, as on the device"""
    with emulating(forward):
        return o.candidate_scores(c['pb']['state'], c['actions'].astype(F32), c['pb']['weights'], c['pb']['inputs_min'], c['pb']['inputs_max'],
                                  c['em'][0], c['ocfg'], c['pb']['scorer'])


def score_stand_in(O, A, variant, order=0):
    return scores_under(score_case(O, A, variant), functools.partial(emu32, order=order))


SCORER_SHAPE = dict(N=96, H=8, P=5, E=5, k=9, I=1)           # tests/test_gpu_parity.py test_rollout_scorer_branches' shape
SCORER_POST = 0.5
SCORER_NOISE_SEED = 12
# Chosen on the CPU (tests/test_bf16_bars_cpu.py re-checks it): 40 populations of 96 are small enough for ONE candidate whose score a
# bf16 tie moved to reach RATIO on the RMS bar, so the seed must keep every stand-in of stand_ins() — 24 chunk orders and the four
# fine-grained sums — inside every bar on all 40 cases.  Of the seeds 7, 9, 10, 11, 12 only 9 and 12 do (largest RMS ratio 0.045 and
# 0.030; at most 9.4 % near, at least 83.3 % flip-free at 12).  Seeds 7, 10 and 11 put a fine-grained stand-in at 0.056 - 0.086 on the
# two_kinds / three_kinds / active_reward_clip cases of obs 60 — and at seed 10 the device sat at 0.056 on active_reward_clip obs 60
# (RMS 6.67e-6 against 1.20e-4: one candidate of 95 moved by 6.5e-5; median and 90th-percentile ratios 0.0005 and 0.0007).


@functools.lru_cache(maxsize=None)
def scorer_case(case, obs, variant):
    """One branch of the scorer (helpers.SCORER_CASES) under bf16: planning mode on explicit noise, as score_case.  For the safe
    objective also `costs` [H, P N] — the done-masked per-step cost of every row on the EMULATION's trajectory (safe_cem_mpc.py:89:
    done OR-ed first) — and `row_clear`, the rows farther than helpers.NEAR from every threshold there."""
    pb = hp.scorer_problem(case, obs)
    n = SCORER_SHAPE
    ea, em, _ = hp.noise(n['I'], n['N'], n['H'], 2, n['P'], obs, seed=SCORER_NOISE_SEED)
    ocfg, _ = hp.configs(pb, variant=variant, post=SCORER_POST, **n)
    c = _score_case(pb, ea, em, ocfg)
    if variant == 'safe':
        traj, sp = c['traj'], pb['scorer']
        done = np.zeros(traj.shape[0], bool)
        costs = np.zeros((n['H'], traj.shape[0]))
        for t in range(n['H']):
            done |= o.reward(traj[:, t], traj[:, t + 1], sp)[1]
            costs[t] = o.cost(traj[:, t], sp) * (1.0 - done)
        c.update(costs=costs, row_clear=o.threshold_margins(traj, sp) > hp.NEAR)
    return c


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
