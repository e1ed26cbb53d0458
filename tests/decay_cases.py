"""Per-iteration population sizes and the mean candidate (cem_planner_set_population_schedule, cem_planner_set_mean_candidate;
DESIGN.md 4.13): the case table tests/test_gpu_population_decay.py runs on the device and tests/test_decay_cases_cpu.py checks on the
host, and the oracle's replay of a scheduled plan.  Plain data and small helpers; importable without a GPU or torch.

Base shape: N = 64, k = 8, I = 3, units 32, P = E = 5, H = 5, obs 10 / act 5 (two action quads, not lean-eligible); every case runs in
a second or two.  What each case is there for:
  lean             obs 12 / act 2, depth 4, one chunk per tile: every iteration reports the lean path
  ragged           populations that are no multiple of the 16-row chunk
  to_k             the last iteration has every candidate elite (n = k)
  grow             a schedule that is not monotone (and whose first iteration is not the widest)
  split_members    N 66, P 2, E 3: the row-to-member map (p n + j) / (P n / E) puts the member boundaries inside tiles, elsewhere per n
  segments         obs 60, N 40, E 2, k 4, rollout_segments = 2: floating horizon segments, another number of floating tiles per iteration
  two_blocks_safe  obs 70 / act 6, the safe objective: two input blocks per wave
  cost             the cost objective
  wide256          a 256-unit handle (cem_rollout_wide.h)
  bf16x3           the split-product rollout (cem_rollout_split.h)
oracle_seeds: noise seeds (hp.noise) for which, in the fp32 oracle's replay, the k-th and (k + 1)-th scores differ by more than
ORACLE_GAP in every iteration with n[it] > k — tests/test_decay_cases_cpu.py recomputes that on the host — so that rounding
differences between the device and the oracle cannot move a candidate across the cut."""
import collections

import numpy as np

from ethz_safe_learning_amd.planner import mean_candidate
from tests import helpers as hp

F, U = np.float32, np.uint32
N, K, I, UNITS, H = 64, 8, 3, 32, 5
ORACLE_GAP = 1e-4                      # five times the score bar of tests/test_gpu_parity.py / tests/test_gpu_whole_plan.py (2e-5)
BASE_SCHEDULE = (64, 48, 32)

Case = collections.namedtuple('Case', 'name obs act depth units precision variant N P E k H schedule segments rc lean oracle_seeds')


def _cases():
    out = []

    def add(name, schedule=BASE_SCHEDULE, obs=10, act=5, variant='cem', depth=4, units=UNITS, precision='fp32', n=N, P=5, E=5, k=K,
            segments=0, rc=0, lean=False, oracle_seeds=()):
        out.append(Case(name, obs, act, depth, units, precision, variant, n, P, E, k, H, tuple(schedule), segments, rc, lean,
                        tuple(oracle_seeds)))

    add('lean', (64, 48, 32), obs=12, act=2, rc=1, lean=True, oracle_seeds=(1, 2))
    add('ragged', (64, 37, 21), oracle_seeds=(1, 2))
    add('to_k', (64, 16, 8), oracle_seeds=(1,))
    add('grow', (32, 64, 48), oracle_seeds=(1,))
    add('split_members', (66, 45, 30), n=66, P=2, E=3, oracle_seeds=(1,))
    add('segments', (40, 24, 8), obs=60, act=2, n=40, P=2, E=2, k=4, segments=2, rc=1, oracle_seeds=(1,))
    add('two_blocks_safe', obs=70, act=6, variant='safe', oracle_seeds=(1,))
    add('cost', variant='cost')
    add('wide256', units=256)
    add('bf16x3', precision='bf16x3')
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
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
    """What hp.configs takes for the case."""
    kw = dict(N=case.N, H=case.H, P=case.P, E=case.E, k=case.k, I=I, variant=case.variant, noise=0.01, post=0.3, chunks_per_tile=case.rc,
              rollout_segments=case.segments, precision=case.precision)
    kw.update(over)
    return kw


def admissible(case):
    """Whether the case's schedule is one cem_planner_set_population_schedule takes: `iterations` entries, each in n_elite .. n_samples
    with particles * n a multiple of ensemble_size."""
    return len(case.schedule) == I and all(case.k <= n <= case.N and (case.P * n) % case.E == 0 for n in case.schedule)


def pad_layout(case):
    """(pad_floats, pad_shift) of the padded action quads (cem_device.h RolloutParams::act_pad): action a of (n, t) is word
    pad_shift + a of the pad_floats words of (n, t); the rest are zero."""
    q0 = case.obs // 4
    nq = (case.obs + case.act + 3) // 4 - q0
    return 4 * nq, case.obs - 4 * q0


def pad_offset(actions_offset, case):
    """Byte offset of act_pad in the workspace: the 256-byte aligned end of `actions` (cem_capi.hip make_layout)."""
    end = actions_offset + case.N * case.H * case.act * 4
    return (end + 255) & ~255


def cut_noise(case, ea, em, it, n=None):
    """What iteration `it` of a scheduled plan reads of the caller's tensors ea [I, N, H, A] and em [I, H, P N, O] (cem_mpc.h): rows
    j < n of slab `it` of ea, and the LEADING H P n O floats of slab `it` of em as [H, P n, O]."""
    n = case.schedule[it] if n is None else n
    rows = case.P * n
    return (np.ascontiguousarray(ea[it][:n]),
            np.ascontiguousarray(em[it].reshape(-1)[:case.H * rows * case.obs].reshape(case.H, rows, case.obs)))


# ---- the oracle's replay ------------------------------------------------------------------------------------------------------------
def oracle_plan(case, noise_seed, with_mean=False, schedule=None):
    """The fp32 oracle's plan of the case under its schedule, on hp.noise(noise_seed) cut as the contract says: per iteration, sample
    n[it] candidates -> (the mean candidate in the last one) -> scores -> select and refit.  -> (action, best score, iterations,
    trace); a trace entry holds actions, scores, elite, mu, sigma."""
    import dataclasses
    from oracle import cem_oracle as o
    assert case.variant in ('cem', 'safe')
    schedule = case.schedule if schedule is None else schedule
    pb = problem(case)
    ocfg, _ = hp.configs(pb, **config_kwargs(case))
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.P, case.obs, seed=noise_seed)
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    mu = np.broadcast_to(mu0, (case.H, case.act)).astype(F).copy()
    sigma = np.broadcast_to(sg0, (case.H, case.act)).astype(F).copy()
    best, best_score = np.zeros(case.act, F), F(-np.inf)
    trace = []
    for it in range(I):
        n = schedule[it]
        cfg_it = dataclasses.replace(ocfg, n_samples=n)
        ea_it, em_it = cut_noise(case, ea, em, it, n)
        actions = o.sample_actions(mu, sigma, lb, ub, ea_it)
        if with_mean and it == I - 1:
            actions = mean_candidate(actions, mu, lb, ub)
        scores = o.candidate_scores(pb['state'], actions, pb['weights'], pb['inputs_min'], pb['inputs_max'], em_it, cfg_it, pb['scorer'])
        mu, sigma, best, best_score, elite, stop = o.select_and_refit(scores, actions, mu, sigma, best, best_score, cfg_it)
        trace.append(dict(actions=actions, scores=scores, elite=elite, mu=mu.copy(), sigma=sigma.copy()))
        if stop:
            break
    return best + eo * F(ocfg.noise_stddev), best_score, len(trace), trace


def oracle_gaps(trace, k):
    """Per iteration the score gap at the k-th place of the population (inf where the population IS k)."""
    out = []
    for t in trace:
        s = np.sort(np.asarray(t['scores'], np.float64))[::-1]
        out.append(s[k - 1] - s[k] if s.size > k else np.inf)
    return out
