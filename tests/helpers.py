"""Shared builders for the parity tests: one synthetic problem -> (oracle config, planner config)."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import cem_oracle as o

from ethz_safe_learning_amd import PlannerConfig, ScorerConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'ethz_safe_learning_amd', 'csrc')


def device_assembly():
    """The device ISA of csrc/cem_capi.hip as text, compiled with the Makefile's own flags (hipcc -S --cuda-device-only; cached under
    /tmp on the hash of the device sources).  Skips the calling test where there is no hipcc."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    flags = makefile_flags()
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(CSRC, f), 'rb').read())
    h.update(open(os.path.join(ROOT, 'include', 'cem_mpc.h'), 'rb').read())
    out = '/tmp/cem_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(CSRC, 'cem_capi.hip')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def unit_assembly(unit_file_name):
    """The device ISA of one translation unit of csrc (cem_task_score.hip, ...) as text, with the Makefile's flags, cached under /tmp
    on the hash of the device sources as device_assembly's is.  Without the compiler the calling test FAILS: the library the tests
    load was built by it."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc), 'no hipcc at %s: %s cannot be compiled for its resource check' % (hipcc, unit_file_name)
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(CSRC, f), 'rb').read())
    h.update(open(os.path.join(ROOT, 'include', 'cem_mpc.h'), 'rb').read())
    out = '/tmp/%s_isa_%s.s' % (os.path.splitext(unit_file_name)[0], h.hexdigest()[:16])
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(CSRC, unit_file_name)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


# What tests/golden/task_kernel_mnemonics.json counts per kernel: memory, LDS, DPP and lane-read instructions and all fp32 arithmetic.
PINNED_MNEMONICS = r'^global_|^ds_|_dpp|^v_readlane|^v_readfirstlane|^v_\w+_f32'


def mnemonic_counts(body):
    """{'total': instructions, 'counts': {mnemonic: n}} of a kernel's instruction lines (kernel_bodies), the mnemonics that match
    PINNED_MNEMONICS."""
    counts = {}
    for line in body:
        m = line.split()[0]
        if re.search(PINNED_MNEMONICS, m):
            counts[m] = counts.get(m, 0) + 1
    return {'total': len(body), 'counts': dict(sorted(counts.items()))}


def template_instance(mangled):
    """_Z21cem_task_zones_kernelILi1ELb0EEv10TaskParams -> 'cem_task_zones_kernel<1, false>' (an <int, bool> kernel template)."""
    m = re.search(r'ILi(\d+)ELb([01])EE', mangled)
    return '%s<%s, %s>' % (kernel_function_name(mangled), m.group(1), 'true' if m.group(2) == '1' else 'false')


def kernel_bodies(isa, pattern):
    """{mangled name: [instruction lines]} of the kernels whose name matches."""
    out = {}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\.Lfunc_end', isa, re.M | re.S):       # (to the end of the function: a kernel may hold early s_endpgm's)
        if re.search(pattern, m.group(1)):
            out[m.group(1)] = [l.split(';')[0].strip() for l in m.group(2).splitlines() if l.strip() and not l.lstrip().startswith((';', '.'))]
    return out


def kernel_meta(isa, pattern, keys=('vgpr_count', 'vgpr_spill_count', 'private_segment_fixed_size')):
    """{mangled name: {key: value}} from the code-object metadata, for the integer `keys` of a kernel's entry (by default vgpr_count,
    vgpr_spill_count, private_segment_fixed_size).  An entry is one item of the amdhsa.kernels list; its keys are in alphabetical order,
    so some (group_segment_fixed_size) stand in front of .name and some behind it."""
    out = {}
    for entry in re.split(r'\n  - ', isa[isa.index('amdhsa.kernels:'):])[1:]:
        m = re.search(r'\.name:\s+(_Z\w+)', entry)
        if m and re.search(pattern, m.group(1)):
            d = {}
            for k in keys:
                mm = re.search(r'^\s+\.%s:\s+(\d+)' % k, entry, re.M)
                d[k] = int(mm.group(1)) if mm else None
            out[m.group(1)] = d
    return out


# The four score kernels of csrc/cem_score.h, by function name (the mangled names carry the parameter type).
SCORE_KERNELS = ('cem_reduce_kernel', 'cem_constraint_reduce_kernel', 'cem_constraint_tail_kernel', 'cem_constrained_budget_kernel')
# Kernels added since warm start that are neither the trainer's nor the forward pass's (tests/test_warm_capi_cpu.py admits exactly these
# beside tests/golden/kernel_registers_before_warm_start.json), by function name.
KERNELS_SINCE_WARM_START = ('cem_pack_fp32_kernel', 'cem_pack_split_kernel', 'cem_pack_wide_kernel', 'cem_pack_bias_kernel',
                            'cem_constraint_reduce_kernel', 'cem_constraint_tail_kernel', 'cem_constrained_budget_kernel', 'cem_constraint_refit_kernel')


def kernel_function_name(mangled):
    """_Z17cem_reduce_kernel12ReduceParams -> cem_reduce_kernel (a plain or templated function at global scope; any other name comes back as it is)."""
    m = re.match(r'_Z(\d+)', mangled)
    return mangled[m.end():m.end() + int(m.group(1))] if m else mangled      # (a nested name, _ZN...: as it is)


def makefile_flags():
    """The device compile flags of csrc/Makefile (without the link flags)."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    return [f for f in re.search(r'^FLAGS\s*:=\s*(.*)$', mk, re.M).group(1).replace('$(ARCH)', 'gfx950').split() if f not in ('-fPIC', '-shared')]


def train_config(D, O, U, L, E, act=0, rate=0.0, batch_size=64):
    """A cem_train_config_t with Keras' Adam constants (mlp_ensemble.py:113-117) for the CPU-side checks of the training ABI."""
    from ethz_safe_learning_amd import _capi
    c = _capi.CemTrainConfig()
    c.abi_version = _capi.CEM_ABI_VERSION
    c.inputs_dim, c.outputs_dim, c.units, c.n_layers, c.ensemble_size = D, O, U, L, E
    c.batch_size, c.activation, c.dropout_rate = batch_size, act, rate
    c.beta1, c.beta2, c.epsilon, c.clipvalue = 0.9, 0.999, 1e-5, 1.0
    return c


def make_problem(obs_dim=60, act_dim=2, E=5, n_layers=4, seed=1234, bias_noise=0.05, units=128, **kw):
    pb = o.synthetic_problem(obs_dim=obs_dim, act_dim=act_dim, ensemble_size=E, units=units, n_layers=n_layers, seed=seed, **kw)
    if bias_noise:
        rng = np.random.default_rng(seed + 999)
        for w in pb['weights']:
            for b in w['b']:
                b[:] = rng.normal(0, bias_noise, b.shape).astype(np.float32)
            w['b_mu'][:] = rng.normal(0, 0.01, obs_dim).astype(np.float32)
            w['b_var'][:] += rng.normal(0, 0.3, obs_dim).astype(np.float32)
    return pb


def with_action_bounds(pb, low, high):
    """The same problem with another action Box (MpcPolicy.sampling_params, mpc_policy.py:45-57): per-dimension (low, high), or a Box
    with an infinite bound anywhere — `is_bounded()` is then False and EVERY dimension takes the +-100 / 0 / 100 branch.  The
    normaliser's action columns are the Box when it is bounded and the range the samples then cover (+-100) when it is not — the data
    range TransitionModel._fit_statistics falls back to (transition_model.py:42-50) — so scaled inputs stay O(1)."""
    low, high = np.asarray(low, np.float32), np.asarray(high, np.float32)
    A = pb['low'].shape[0]
    assert low.shape == (A,) and high.shape == (A,)
    pb = dict(pb)
    pb['low'], pb['high'] = low, high
    O = pb['state'].shape[0]
    imin, imax = pb['inputs_min'].copy(), pb['inputs_max'].copy()
    bounded = bool(np.all(np.isfinite(low)) and np.all(np.isfinite(high)))
    imin[O:] = low if bounded else np.float32(-100.0)
    imax[O:] = high if bounded else np.float32(100.0)
    pb['inputs_min'], pb['inputs_max'] = imin, imax
    return pb


def random_action_bounds(rng, A):
    """(kind, low, high): 'unit' Box(-1, 1), 'asym' per-dimension bounds of mixed sign / width (one dimension may be a single point),
    'unbounded' (all infinite) or 'mixed' (some infinite: the reference then ignores the finite ones too)."""
    kind = str(rng.choice(['unit', 'asym', 'asym', 'asym', 'asym', 'unbounded', 'mixed', 'mixed']))
    if kind == 'unit':
        return kind, -np.ones(A, np.float32), np.ones(A, np.float32)
    centre = rng.uniform(-2.0, 2.0, A)
    half = rng.uniform(0.05, 1.5, A)
    if kind == 'asym' and A > 1 and rng.random() < 0.25:
        half[int(rng.integers(0, A))] = 0.0                 # low == high: sigma0 = 0, every sample of that dimension is the bound
    low, high = (centre - half).astype(np.float32), (centre + half).astype(np.float32)
    if kind == 'unbounded':
        low[:], high[:] = -np.inf, np.inf
    elif kind == 'mixed':
        j = int(rng.integers(0, A))
        if rng.random() < 0.5:
            high[j] = np.inf
        else:
            low[j] = -np.inf
    return kind, low, high


def configs(pb, N, H, P, E, k, I=3, variant='cem', thr=-1.0, noise=0.0, post=0.3, smoothing=0.0,
            sampling=True, scale=True, world_size=1, rank=0, chunks_per_tile=0, use_graph=False, rollout_segments=0, select_mode=0, precision='fp32'):
    sp = pb['scorer']
    O, A = pb['state'].shape[0], pb['low'].shape[0]
    # CEM_TEST_PRECISION=bf16x3: run every eligible case (units <= 128, relu) of the suites on the split-product rollout (a one-off coverage run)
    if os.environ.get('CEM_TEST_PRECISION') and pb['weights'][0]['W'][0].shape[1] <= 128 and pb['weights'][0].get('activation', 'relu') == 'relu':
        precision = os.environ['CEM_TEST_PRECISION']
    ocfg = o.PlanConfig(horizon=H, iterations=I, n_samples=N, n_elite=k, particles=P, ensemble_size=E, smoothing=smoothing,
                        stddev_threshold=thr, noise_stddev=noise, variant=variant, posterior_mean_threashold=post,
                        scale_features=scale, sampling_propagation=sampling)
    pcfg = PlannerConfig(obs_dim=O, act_dim=A, ensemble_size=E, particles=P, n_samples=N, horizon=H, n_elite=k, iterations=I,
                         scorer=ScorerConfig(goal_slice=sp.goal_slice, observe_goal_lidar=sp.observe_goal_lidar,
                                             lidar_max_dist=sp.lidar_max_dist, goal_size=sp.goal_size,
                                             reward_distance=sp.reward_distance, reward_goal=sp.reward_goal,
                                             reward_clip=sp.reward_clip, constrain_indicator=sp.constrain_indicator,
                                             cost_kinds=list(sp.cost_kinds)),
                         act_low=pb['low'], act_high=pb['high'], n_layers=len(pb['weights'][0]['W']), units=pb['weights'][0]['W'][0].shape[1],
                         activation=pb['weights'][0].get('activation', 'relu'),
                         smoothing=smoothing,
                         stddev_threshold=thr, noise_stddev=noise, variant=variant, posterior_mean_threashold=post,
                         sampling_propagation=sampling, scale_features=scale, world_size=world_size, rank=rank,
                         chunks_per_tile=chunks_per_tile, use_graph=use_graph, rollout_segments=rollout_segments, select_mode=select_mode,
                         precision=precision)
    return ocfg, pcfg


def noise(I, N, H, A, P, O, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((I, N, H, A)).astype(np.float32),
            rng.standard_normal((I, H, P * N, O)).astype(np.float32),
            rng.standard_normal((A,)).astype(np.float32))


def make_planner(pb, pcfg):
    from ethz_safe_learning_amd import CemPlanner
    pl = CemPlanner(pcfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


class Arrays:
    """The per-candidate arrays of a handle as flat byte views, and the bytes of each that a population of n owns: the leading ones."""

    def __init__(self, pl, case):
        import torch as t
        from tests import decay_cases as dc
        self.pl, self.case, self.t = pl, case, t
        pf, _ = dc.pad_layout(case)
        N, Hh, A, P = case.N, case.H, case.act, case.P
        lay = pl.layout
        self.spec = dict(actions=(lay.actions, N * Hh * A * 4, Hh * A * 4), act_pad=(dc.pad_offset(lay.actions, case), N * Hh * pf * 4, Hh * pf * 4),
                         scores=(lay.scores_local, N * 4, 4), returns=(lay.returns, P * N * 4, P * 4), costs=(lay.costs, Hh * P * N, Hh * P))
        self.saved = {}

    def view(self, key):
        off, total, _ = self.spec[key]
        return self.pl._ws_view[off:off + total]

    def lead(self, key, n):
        return self.spec[key][2] * n

    def get(self, key, n, dtype=None):
        """The leading bytes of `key` a population of n owns, as numpy (dtype: float32 unless uint8 is asked for)."""
        self.pl.synchronize()
        b = self.view(key)[:self.lead(key, n)].cpu().numpy().copy()
        return b if dtype == np.uint8 else b.view(np.float32)

    def poison(self, n):
        """Everything beyond the leading n entries of every array becomes 0xFF bytes (what was there is kept for `check`)."""
        self.pl.synchronize()
        with self.pl.stream_context():
            for key in self.spec:
                tail = self.view(key)[self.lead(key, n):]
                self.saved[key] = tail.clone()
                tail.fill_(0xFF)
        self.pl.synchronize()

    def check(self, n, what):
        """The poison is intact; then what it covered comes back (the padding words of act_pad are zeros no kernel ever rewrites)."""
        self.pl.synchronize()
        with self.pl.stream_context():
            for key in self.spec:
                tail = self.view(key)[self.lead(key, n):]
                assert bool((tail == 0xFF).all()), '%s: %s beyond the leading %d entries was written' % (what, key, n)
                tail.copy_(self.saved[key])
        self.pl.synchronize()


def elite_sets_equal_modulo_ties(scores, elite_a, elite_b, tol):
    """Two top-k sets agree if every candidate in the symmetric difference scores within tol of the k-th score."""
    a, b = set(int(x) for x in elite_a), set(int(x) for x in elite_b)
    if a == b:
        return True
    kth = np.sort(scores)[::-1][len(a) - 1]
    return all(abs(float(scores[i]) - float(kth)) <= tol for i in a ^ b)


# --------------------------------------------------------------------------------------------------------------------
# scorer branches of SafetyGymStateScorer (safety_gym.py:145-176): several constrained kinds, the non-indicator sum,
# observe_goal_dist instead of the goal lidar, no / active reward clip
# --------------------------------------------------------------------------------------------------------------------
# lidar-like slices per observation width: goal lidar, then the four cost kinds in the reference's order vases, hazards,
# pillars, gremlins (safety_gym.py:148-163), and the feature used as goal_dist.  obs 60 (obs+act <= 64: one input block per
# wave) reuses PointGoal1's layout and squeezes pillars / gremlins into the 3-wide gyro / velocimeter slots; obs 84 (two
# input blocks per wave) has room for two more 8-bin lidars.
SCORER_LAYOUTS = {
    60: dict(goal=(3, 19), kinds=[(41, 57), (22, 38), (19, 22), (57, 60)], goal_dist=0),
    84: dict(goal=(3, 19), kinds=[(41, 57), (22, 38), (64, 72), (72, 80)], goal_dist=60),
}
SCORER_SIZE_FRAC = 0.7
SCORER_CASES = {
    # name: (which of the four kinds are constrained, overrides)
    'two_kinds': dict(kinds=[0, 1]),
    'three_kinds': dict(kinds=[0, 1, 2]),
    'four_kinds': dict(kinds=[0, 1, 2, 3]),
    'four_kinds_sum': dict(kinds=[0, 1, 2, 3], constrain_indicator=False),
    'one_kind_sum': dict(kinds=[1], constrain_indicator=False),
    'no_cost_kinds': dict(kinds=[]),
    'goal_dist': dict(kinds=[1], observe_goal_lidar=False),                                  # observe_goal_dist (safety_gym.py:172-174)
    'goal_dist_sum3': dict(kinds=[0, 1, 2], observe_goal_lidar=False, constrain_indicator=False),
    'no_reward_clip': dict(kinds=[1], reward_clip=0.0, reward_goal=25.0),                    # falsy clip: no clipping (safety_gym.py:141)
    'active_reward_clip': dict(kinds=[1], reward_clip=0.02),                                 # |r| exceeds the clip on most steps
}


def scorer_problem(case, obs_dim=60, seed=31, E=5):
    """A problem whose scorer exercises the named branch.  Lidar-like slices get lidar-like state values (closest distances
    straddle the kinds' sizes) and the [0, 1] normaliser."""
    spec, lay = SCORER_CASES[case], SCORER_LAYOUTS[obs_dim]
    pb = make_problem(obs_dim, 2, E, 4, seed=seed)
    rng = np.random.default_rng(seed + 5)
    sp = pb['scorer']
    for lo, hi in [lay['goal']] + lay['kinds']:
        pb['state'][lo:hi] = rng.uniform(0.2, 0.9, hi - lo).astype(np.float32)
        pb['inputs_min'][lo:hi] = 0.0
        pb['inputs_max'][lo:hi] = 1.0
    goal_lidar = spec.get('observe_goal_lidar', True)
    goal_slice = lay['goal'] if goal_lidar else (lay['goal_dist'], lay['goal_dist'] + 1)
    if not goal_lidar:
        pb['state'][goal_slice[0]] = np.float32(0.27)          # goal_dist a little above 0.8 * goal_size: some rollouts reach the goal
    # a kind's size sits just under the closest distance of the real s_0, so predicted states drift in and out of it
    kinds = [(lay['kinds'][i][0], lay['kinds'][i][1],
              float(np.float32(SCORER_SIZE_FRAC * sp.lidar_max_dist * pb['state'][lay['kinds'][i][0]:lay['kinds'][i][1]].min()))) for i in spec['kinds']]
    pb['scorer'] = o.ScorerParams(goal_slice=goal_slice, observe_goal_lidar=goal_lidar,
                                  lidar_max_dist=sp.lidar_max_dist, goal_size=sp.goal_size, reward_distance=sp.reward_distance,
                                  reward_goal=spec.get('reward_goal', sp.reward_goal), reward_clip=spec.get('reward_clip', sp.reward_clip),
                                  constrain_indicator=spec.get('constrain_indicator', True), cost_kinds=kinds)
    return pb


# --------------------------------------------------------------------------------------------------------------------
# scores against the oracle, near-threshold candidates included
# --------------------------------------------------------------------------------------------------------------------
NEAR = 1e-4          # a `<=` comparison whose operands are closer than this may resolve either way within the rollout's rounding


def objective(traj, P, n, sp, variant, post):
    return o.compute_objective_safe(traj, P, n, sp, post) if variant == 'safe' else o.compute_objective_cem(traj, P, n, sp)


def admissible_scores(traj64, P, n, sp, variant, post, delta=2 * NEAR):
    """The oracle's objective under the ways a trajectory's near-threshold comparisons can legitimately resolve: the nominal
    thresholds, and the goal threshold / the cost sizes each moved down or up by `delta` (which flips exactly the comparisons whose
    operands lie within delta of the threshold) — nine score vectors, the nominal one first."""
    import dataclasses
    out = []
    for dg in (0, -1, 1):
        for dc in (0, -1, 1):
            v = dataclasses.replace(sp, goal_size=sp.goal_size + dg * delta / 0.8,
                                    cost_kinds=[(lo, hi, size + dc * delta) for lo, hi, size in sp.cost_kinds])
            out.append(objective(traj64, P, n, v, variant, post))
    return out


def assert_scores_match_oracle(scores_gpu, traj64, P, n, sp, variant, post, atol, what=''):
    """Every candidate's GPU score equals the fp64 oracle's within atol + half an fp32 ulp — candidates with a comparison within NEAR
    of its threshold (rounding may flip it) must equal the oracle's score under one of the admissible resolutions instead of being
    skipped.  Returns (max error over the clear candidates, number of near-threshold candidates, how many of those took a flipped
    outcome)."""
    outs = admissible_scores(traj64, P, n, sp, variant, post)
    ref = outs[0]
    allow = atol + 6e-8 * np.abs(ref)
    err = np.abs(scores_gpu - ref)
    near = o.threshold_margins(traj64, sp).reshape(P, n).min(axis=0) <= NEAR
    clear_bad = np.nonzero(~near & (err > allow))[0]
    assert clear_bad.size == 0, '%s: %d clear candidates differ from the oracle, e.g. %d: gpu %.9g oracle %.9g' % (
        what, clear_bad.size, clear_bad[0], scores_gpu[clear_bad[0]], ref[clear_bad[0]])
    best = np.min(np.stack([np.abs(scores_gpu - r) / (atol + 6e-8 * np.abs(r)) for r in outs]), axis=0)
    near_bad = np.nonzero(near & (best > 1.0))[0]
    assert near_bad.size == 0, '%s: %d near-threshold candidates equal none of the admissible outcomes, e.g. %d: gpu %.9g nominal %.9g' % (
        what, near_bad.size, near_bad[0], scores_gpu[near_bad[0]], ref[near_bad[0]])
    flipped = int((near & (err > allow)).sum())
    return (float(err[~near].max()) if (~near).any() else 0.0), int(near.sum()), flipped
