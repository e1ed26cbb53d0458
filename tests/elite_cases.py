"""Elite carry-over (cem_planner_set_elite_carry): the case table tests/test_gpu_elite_carry.py runs on the device and
tests/test_elite_cases_cpu.py checks on the host, the adversarial score vectors cut from tests/select_cases.py, and the oracle's replay of
a plan with carry-over.  Plain data and small helpers; importable without a GPU or torch.

Every case is small enough to run in a second or two: N = 64, k = 8, I = 3, units 32 unless the case is about something else (the wide
family needs 256 units; the floating-segment case takes the population and ensemble of the existing segment tests, N = 40 and E = 2).
What each case is there for:
  lean_one_quad    obs 12 / act 2, depth 4, one chunk per tile: lean-eligible (the handle must leave the lean path and come back), one action quad
  two_quads        obs 10 / act 5: two action quads, the second partial, pad_shift = 2; the largest shift, H - 1
  two_blocks       obs 70 / act 6: two input blocks per wave; H = 2, where shift 1 is also H - 1; m = 1
  wide256          a 256-unit handle (cem_rollout_wide.h); m = k: every elite is kept
  bf16x3           the split-product rollout (cem_rollout_split.h)
  h1               H = 1: carry-over inside a plan works, across_plans must be refused (no shift fits)
  safe, cost       the other objectives; 'cost' scores are multiples of 1 / P, so the m-th place is usually inside a run of equal scores
  segments         floating horizon segments (an explicit rollout_segments floats every tile)
oracle_seeds: noise seeds (hp.noise) for which, in the fp32 oracle's replay, the k-th and (k + 1)-th scores and the m-th and (m + 1)-th
elite scores differ by more than ORACLE_GAP in every iteration — tests/test_elite_cases_cpu.py recomputes that on the host — so that
rounding differences between the device and the oracle cannot move a candidate across either cut."""
import collections

import numpy as np

from ethz_safe_learning_amd.planner import inject_elites, keep_elites
from tests import helpers as hp
from tests import select_cases as sc

F, U = np.float32, np.uint32
N, K, I, UNITS = 64, 8, 3, 32
ELITE_MAX_K = 4096                     # csrc/cem_elite_carry.h CEM_ELITE_MAX_K: the keep stages 8 bytes per elite in LDS
ORACLE_GAP = 1e-4                      # five times the score bar of tests/test_gpu_parity.py / tests/test_gpu_whole_plan.py (2e-5)

Case = collections.namedtuple('Case', 'name obs act depth units precision variant N E k H m shift segments rc lean oracle_seeds')


def _cases():
    out = []

    def add(name, obs, act, H, m, shift, variant='cem', depth=4, units=UNITS, precision='fp32', n=N, E=5, k=K, segments=0, rc=0, lean=False,
            oracle_seeds=()):
        out.append(Case(name, obs, act, depth, units, precision, variant, n, E, k, H, m, shift, segments, rc, lean, tuple(oracle_seeds)))

    add('lean_one_quad', 12, 2, 5, 3, 1, rc=1, lean=True, oracle_seeds=(2, 3))
    add('two_quads', 10, 5, 5, 3, 4, oracle_seeds=(1,))
    add('two_blocks', 70, 6, 2, 1, 1, variant='safe', oracle_seeds=(2,))
    add('wide256', 12, 2, 5, K, 1, units=256)
    add('bf16x3', 12, 2, 5, 3, 1, precision='bf16x3')
    add('h1', 12, 2, 1, 3, 1)
    add('safe', 12, 2, 5, 3, 2, variant='safe', oracle_seeds=(2,))
    add('cost', 12, 2, 5, 3, 1, variant='cost')
    add('segments', 60, 2, 5, 1, 1, n=40, E=2, k=4, segments=2, rc=1)
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
ACROSS_CASES = [c for c in CASES if c.H > 1]                        # H = 1 refuses across_plans
ORACLE_CASES = [(c, s) for c in CASES for s in c.oracle_seeds]
PLAN_SEED, PLAN_CALL = 5, 3

_PROBLEMS = {}


def problem(case):
    """The case's synthetic problem (cached: weights and state are never written to)."""
    key = (case.obs, case.act, case.E, case.depth, case.units)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = hp.make_problem(case.obs, case.act, case.E, case.depth, seed=77, units=case.units)
    return _PROBLEMS[key]


def config_kwargs(case, **over):
    """What hp.configs takes for the case (P = E)."""
    kw = dict(N=case.N, H=case.H, P=case.E, E=case.E, k=case.k, I=I, variant=case.variant, noise=0.01, post=0.3, chunks_per_tile=case.rc,
              rollout_segments=case.segments, precision=case.precision)
    kw.update(over)
    return kw


def pad_layout(case):
    """(pad_floats, pad_shift) of the padded action quads (cem_device.h RolloutParams::act_pad): action a of (n, t) is word
    pad_shift + a of the pad_floats words of (n, t); the rest are zero."""
    q0 = case.obs // 4
    nq = (case.obs + case.act + 3) // 4 - q0
    return 4 * nq, case.obs - 4 * q0


def pad_offset(actions_offset, case, problems=1):
    """Byte offset of act_pad in the workspace: the 256-byte aligned end of `actions` (cem_capi.hip make_layout)."""
    end = actions_offset + problems * case.N * case.H * case.act * 4
    return (end + 255) & ~255


# ---- adversarial scores for the keep: vectors of tests/select_cases.py cut down to a population of n ---------------------------------
def adversarial_scores(n, k, m):
    """{name: float32 [n]}: what the select may hand the keep at its worst — runs of equal values across the m-th place, both zeros in one
    run, NaNs (every payload of the select's NaN case) and both infinities among the elites."""
    assert 1 <= m <= k < n
    out = {}
    out['all_equal'] = sc.BY_NAME['all_equal'].scores[:n].copy()                     # every place a tie: lowest indices first
    z = sc.BY_NAME['signed_zeros'].scores[:n].copy()                                 # -0.0, +0.0, a negative, ...: the elites are zeros of both signs
    out['signed_zeros'] = z
    if n == 64:
        out['signed_zero_pair'] = sc.BY_NAME['signed_zero_pair'].scores.copy()       # ten positives, then the pair: with k = 11 the cut splits it
    nan_case = sc.BY_NAME['nan'].scores
    nans = nan_case[(nan_case.view(U) & U(0x7fffffff)) > U(0x7f800000)]
    v = sc.BY_NAME['full_span_cut'].scores[:n].copy()                                # +inf at index 5, a band around -100
    v[n - 1] = -np.inf
    out['infinities'] = v
    # NaN below -inf below the rest, and more of them than n - k: NaNs and -inf ARE elites, in key order behind everything finite
    v = np.resize(nans, n).astype(F)
    finite = np.arange(0, n, max(2, n // max(k - 3, 1)))[:max(k - 3, 1)]
    v[finite] = np.linspace(-2.0, 2.0, finite.size).astype(F)
    v[1] = -np.inf
    out['nan_elites'] = v
    # a run of equal values across the m-th place of the elites (select_cases._plant_run at rank m): m - 1 above it, the run, the rest below
    rng = np.random.default_rng(90)
    v = np.round(rng.standard_normal(n), 2).astype(F)
    sc._plant_run(v, m, min(m, 2), 2)
    out['run_across_m'] = v
    w = v.copy()
    sc._plant_run(w, k, min(k, 2), 2)
    out['run_across_k'] = w
    return {name: np.ascontiguousarray(x, F) for name, x in out.items()}


# ---- the oracle's replay ------------------------------------------------------------------------------------------------------------
def oracle_plan(case, noise_seed, m=None):
    """The fp32 oracle's plan of the case with carry-over inside the plan, on hp.noise(noise_seed): sample -> inject -> scores -> select
    and refit -> keep, per iteration.  -> (action, best score, iterations, trace); a trace entry holds actions (after the inject),
    scores, elite, mu, sigma, store."""
    from oracle import cem_oracle as o
    assert case.variant in ('cem', 'safe')
    m = case.m if m is None else m
    pb = problem(case)
    ocfg, _ = hp.configs(pb, **config_kwargs(case))
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.E, case.obs, seed=noise_seed)
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    mu = np.broadcast_to(mu0, (case.H, case.act)).astype(F).copy()
    sigma = np.broadcast_to(sg0, (case.H, case.act)).astype(F).copy()
    best, best_score = np.zeros(case.act, F), F(-np.inf)
    store, trace = None, []
    for it in range(I):
        actions = o.sample_actions(mu, sigma, lb, ub, ea[it])
        if store is not None:
            actions = inject_elites(actions, store, m, 0)
        scores = o.candidate_scores(pb['state'], actions, pb['weights'], pb['inputs_min'], pb['inputs_max'], em[it], ocfg, pb['scorer'])
        mu, sigma, best, best_score, elite, stop = o.select_and_refit(scores, actions, mu, sigma, best, best_score, ocfg)
        store = keep_elites(scores, elite, actions, m)
        trace.append(dict(actions=actions, scores=scores, elite=elite, mu=mu.copy(), sigma=sigma.copy(), store=store))
        if stop:
            break
    return best + eo * F(ocfg.noise_stddev), best_score, len(trace), trace


def oracle_gaps(trace, k, m):
    """Per iteration (score gap at the k-th place of the population, score gap at the m-th place of the elites; inf where m == k)."""
    out = []
    for t in trace:
        s = np.sort(np.asarray(t['scores'], np.float64))[::-1]
        out.append((s[k - 1] - s[k], s[m - 1] - s[m] if m < k else np.inf))
    return out
