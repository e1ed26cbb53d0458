"""Seeded configurations of batched planning (cem_batch_planner_create / cem_planner_plan_batch) for tests/test_gpu_batch_fuzz.py.

Every draw is one a batch handle accepts (validate_batch: one rank, fp32, units <= 128, relu, the one-workgroup select) and sweeps
what the slice addressing of the batched kernels depends on: action dims other than 2 (several wrong strides equal the right one at
A = 2), obs + act on both sides of 64 (one or two input blocks per wave), narrow and odd widths, members that split a particle,
every tile size, forced horizon segments on the single-state side (a batch handle never segments), both samplers, graph and eager,
early stop, output noise, and n_states below the capacity.  tests/test_batch_cases_cpu.py checks on the CPU that every case is
accepted and that the draws cover these corners."""
import numpy as np

from oracle import cem_oracle as o
from tests import helpers as hp

A_DIMS = (1, 2, 3, 4, 5, 7, 8, 12)
OBS_DIMS = (9, 31, 60, 61, 63, 70, 100)           # 60 + A <= 64 for A <= 4; 61 / 63 / 70 / 100 cross 64 for larger A
UNITS = (16, 17, 33, 64, 100, 127, 128)
MAX_BATCH = (1, 2, 3, 5, 8, 17)
ROW_STEPS = 40000                                   # P * N * H of one problem: a case stays well under a second of GPU time
N_MAX = 4096                                        # candidates: the one-workgroup select with its keys in LDS (a batch handle's only form)
ORACLE_ROW_STEPS = 6000                             # ... and the fp64 oracle a second or two of CPU time per problem


def random_batch_case(seed, oracle=False):
    """One configuration as a dict of plain values (printed by every failure: it reproduces the case).  oracle=True: a first-iteration
    case for the fp64 oracle (I = 1, explicit noise, a smaller population, at least two problems so every slice but the first is read)."""
    rng = np.random.default_rng((31000 if oracle else 21000) + seed)
    A = int(rng.choice(A_DIMS))
    O = int(rng.choice(OBS_DIMS))
    E = int(rng.integers(1, 17))
    H = int(rng.integers(1, 51))
    cap = ORACLE_ROW_STEPS if oracle else ROW_STEPS
    split = bool(rng.random() < 0.4)
    if split:                                       # members split particles: P * N divides by E, P < E where E allows it
        P = int(rng.integers(1, min(4, max(1, E - 1)) + 1))
        N = E * int(rng.integers(1, max(1, min(cap // (P * H), N_MAX) // E) + 1))
    else:                                           # whole particles per member
        P = E * int(rng.integers(1, 4))
        N = int(rng.integers(1, max(1, min(cap // (P * H), N_MAX)) + 1))
    k = int(rng.choice([1, 2, N // 10, N // 2, N]))
    c = dict(seed=int(seed), O=O, A=A, E=E, P=P, N=N, H=H, k=min(max(k, 1), N), split=split,
             L=int(rng.integers(1, 6)), units=int(rng.choice(UNITS)),
             I=1 if oracle else (1 if rng.random() < 0.15 else int(rng.integers(2, 7))),
             variant=str(rng.choice(['cem', 'safe'])), post=float(rng.choice([0.15, 0.3, 0.5])),
             smoothing=float(rng.choice([0.0, 0.1, 0.5])),
             noise=float(rng.choice([0.0, 0.02, 0.1])) if not oracle else float(rng.choice([0.0, 0.05, 0.05])),
             sampling=bool(rng.random() < 0.8), scale=bool(rng.random() < 0.8),
             rc=int(rng.integers(0, 5)), seg=int(rng.choice([0, 0, 1, 2, 3])),
             sampler=str(rng.choice(['tile', 'kernel'])), use_graph=bool(rng.random() < 0.5) and not oracle)
    c['box'], low, high = hp.random_action_bounds(rng, A)
    c['low'], c['high'] = [float(x) for x in low], [float(x) for x in high]
    sigma0 = o.sampling_params(low, high)[3]
    # early stop: off, or a threshold on mean(sigma) a refit of the first iterations reaches (the problems then stop on their own)
    c['thr'] = -1.0 if rng.random() < 0.5 else float(np.float32(rng.choice([0.3, 0.6, 0.9]) * float(sigma0.mean())))
    if oracle:
        c['max_batch'] = int(rng.choice([2, 3, 5]))
        c['n_states'] = int(rng.integers(2, c['max_batch'] + 1))
    else:
        c['max_batch'] = int(rng.choice(MAX_BATCH))
        c['n_states'] = int(rng.integers(1, c['max_batch'] + 1))
    return c


def problem(c):
    """The synthetic problem of a case (weights, normaliser, state, scorer) with the case's action Box."""
    pb = hp.make_problem(c['O'], c['A'], c['E'], c['L'], seed=700 + c['seed'], units=c['units'])
    return hp.with_action_bounds(pb, np.array(c['low'], np.float32), np.array(c['high'], np.float32))


def configs(pb, c):
    """(oracle config, planner config) of a case."""
    return hp.configs(pb, N=c['N'], H=c['H'], P=c['P'], E=c['E'], k=c['k'], I=c['I'], variant=c['variant'], thr=c['thr'],
                      noise=c['noise'], post=c['post'], smoothing=c['smoothing'], sampling=c['sampling'], scale=c['scale'],
                      chunks_per_tile=c['rc'], use_graph=c['use_graph'], rollout_segments=c['seg'])


def states(pb, n, seed, spread=0.05):
    """n observations: row 0 the problem's own state, the others perturbed (distinct problems)."""
    rng = np.random.default_rng(seed)
    st = np.repeat(pb['state'][None], n, 0).astype(np.float32)
    st[1:] += rng.normal(0.0, spread, st[1:].shape).astype(np.float32)
    return st


def calls(n, seed):
    """n distinct call numbers, some above 2^32 (the Philox key's high word)."""
    rng = np.random.default_rng(seed)
    return rng.choice(1 << 40, size=n, replace=False).astype(np.uint64)


N_CASES = 32                                        # single-vs-batch cases of the default suite (x CEM_FUZZ_SCALE)
N_ORACLE_CASES = 12


def isolation_seeds():
    """Generator seeds of the isolation tests (leave-one-out, duplicates, the untouched tail): the first four cases with room for at
    least three problems, one of them (the first such) with an action dimension of 3, 5 or 12."""
    roomy = [s for s in range(1000) if random_batch_case(s)['max_batch'] >= 3]
    odd = next(s for s in roomy if random_batch_case(s)['A'] in (3, 5, 12))
    return sorted(roomy[:4] if odd in roomy[:4] else roomy[:3] + [odd])
