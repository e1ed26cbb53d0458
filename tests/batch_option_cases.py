"""Option combinations on a BATCH handle: the generated case table tests/test_gpu_batch_option_fuzz.py runs on the device
and tests/test_batch_option_cases_cpu.py checks on the host.  Plain data and NumPy; importable without a GPU or torch.

A batch handle (cem_batch_planner_create) admits seven of the ten options of tests/composed_cases.py — tail, budget, softmax, mixed, carry
(inside a plan only), track, warm — and refuses schedules, the mean candidate, tasks, across-plans carry and bf16 (admit()'s f.batch line in
csrc/cem_plan_options.h, validate_batch in csrc/cem_capi.hip).  The cases are composed_cases.Case / Options values, so apply_options,
problem, config_kwargs, on and admitted work on them unchanged, and every case is also a single-state case of the composed fuzz.

batch_case_for(seed) -> (case, max_batch, calls_plan): seeds 0 .. 19 force one of the 20 option pairs (all pairs of the seven but
tail x budget) and draw every other option with probability 0.3; seeds 20 .. 22 switch on everything that can be on at once, on a cem handle
(tail), a safe handle (budget) and a cost handle.  Shapes are the smallest at which the per-problem addressing can still go wrong: A in
1 / 3 / 5 / 7 / 8 (several wrong strides give the right address at A = 2, which only the lean-eligible seeds keep), N 24 .. 96 with values
that are no multiple of the 16-row chunk, H 2 .. 6, I 2 .. 4, E 1 .. 4, P <= 6, O in 9 / 12 / 31 / 60 / 70, units 32 / 64 / 100 / 128,
depth 2 .. 4, chunks_per_tile 0 .. 2, rollout_segments 0 / 2 (the SINGLE side only: a batch handle never segments), and every fourth seed
the lean-eligible shape (obs 12 / act 2, depth 4, one chunk per tile: the single side rolls out on the lean kernels where its options allow,
the batch side never does).  max_batch is 2 / 3 / 5, graph and eager alternate.

calls_plan describes three consecutive plan_batch calls: a full batch; fewer problems, under a permuted slot map when warm start is on; a
full batch again under another permutation, one slot's carry reset first when warm start is on.  States are distinct per slot and per
call and spread widely around the problem's own (STATE_SPREAD), call numbers are distinct with some above 2^32.

The early-stop threshold is off on about half of the cases and otherwise a fraction of the Box's mean sigma0 (as tests/batch_cases.py
draws it).  The forced pairs with warm start and the "everything" handles always take a threshold (STAGGER_FRACTION), the 'keep' sigma rule,
a shift of one step, two or three elites and little smoothing: sigma falls fast, and a slot whose carry was reset restarts from the Box
next to slots that start from a kept, narrow sigma, so in ONE launch some problems are done while others still run — the launches
tests/golden/batch_option_staggered.json lists (recorded from a device run: the seeds and the call index, nothing else)."""
import collections
import itertools
import json
import os

import numpy as np

from tests import composed_cases as cp
from tests import helpers as hp

F = np.float32
BATCH_OPTIONS = ('tail', 'budget', 'softmax', 'mixed', 'carry', 'track', 'warm')
PAIRS = [p for p in itertools.combinations(BATCH_OPTIONS, 2) if p != ('tail', 'budget')]
assert len(PAIRS) == 20
EVERYTHING = ('cem', 'safe', 'cost')                  # seeds 20 .. 22
N_SEEDS = len(PAIRS) + len(EVERYTHING)
A_DIMS = (1, 3, 5, 7, 8)                              # of the seeds that are not lean-eligible (those have A = 2)
OBS_DIMS = (9, 12, 31, 60, 70)
UNITS = (32, 64, 100, 128)
MAX_BATCH = (2, 3, 5)
THR_FRACTIONS = (0.3, 0.6, 0.9)                       # of the Box's mean sigma0 (tests/batch_cases.py)
STAGGER_FRACTION = 0.45                               # ... of the cases that are built to stop at different iterations (_draw)
STATE_SPREAD = 0.5                                    # std of the states around the problem's own: the problems differ in where they stop
BATCH_CAP = 256                                       # include/cem_mpc.h CEM_MAX_BATCH
SELECT_MAX_N = 4096                                   # the one-workgroup select, a batch handle's only form (tests/batch_cases.py N_MAX)
STAGGERED_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'batch_option_staggered.json')

# One plan_batch call: n problems, row b on carry slot slots[b] (None: the map stays as it is, initially row b -> slot b), `reset` the slot
# whose carry is reset first (None: none), states [n, O], call numbers uint64 [n]
Call = collections.namedtuple('Call', 'n slots reset states calls')
CallsPlan = collections.namedtuple('CallsPlan', 'use_graph plan_seed calls')


def batch_admitted(case, max_batch):
    """composed_cases.admitted plus what a batch handle adds: admit()'s f.batch line (no schedule, no mean candidate, no across-plans
    carry), its task line (no task on a batch handle), and validate_batch (1 .. CEM_MAX_BATCH problems, fp32, units <= 128, the
    one-workgroup select)."""
    o = case.opt
    if not cp.admitted(case):
        return False
    if o.schedule is not None or o.mean or o.task is not None or (o.keep is not None and o.keep.across):
        return False
    if case.precision != 'fp32' or case.units > 128 or case.N > SELECT_MAX_N:
        return False
    return 1 <= int(max_batch) <= BATCH_CAP


def slot_rows(call, max_batch):
    """The carry slot of every row of a call: its map, or row b -> slot b."""
    return tuple(range(call.n)) if call.slots is None else tuple(call.slots)


def _draw(seed, rng, forced, everything):
    lean = everything is None and seed % 4 == 0
    # the forced warm pairs and the "everything" handles stop early under the 'keep' rule (the module docstring): few elites and little
    # smoothing let sigma fall fast, so that a cold slot needs at least two iterations to pass a threshold its warm neighbours start near
    stagger = 'warm' in forced or everything is not None
    A = 2 if lean else int(rng.choice(A_DIMS))
    O = 12 if lean else int(rng.choice(OBS_DIMS))
    E = int(rng.integers(1, 5))
    if rng.random() < 0.6:
        P, q = E * int(rng.integers(1, max(1, 6 // E) + 1)), 1                  # whole particles per member
    else:
        P = int(rng.integers(1, 5))                                             # members split particles: P N must divide by E
        q = E // int(np.gcd(P, E))
    N = -(-int(rng.integers(24, 97)) // q) * q
    if lean:
        N = min(96, -(-N // (16 * q)) * 16 * q) if 16 * q <= 96 else N
    N = min(N, 96 // q * q)
    k = int(rng.choice([2, 3] if stagger else [2, 3, max(2, N // 10), max(2, N // 4)]))
    k = min(N, -(-k // q) * q)
    H, I = int(rng.integers(3 if stagger else 2, 7)), int(rng.integers(3 if stagger else 2, 5))
    units = int(rng.choice(UNITS))
    depth = 4 if lean else int(rng.integers(2, 5))
    variant = everything if everything else ('cem', 'safe', 'cost')[seed % 3]
    if 'budget' in forced:
        variant = 'safe'
    elif 'tail' in forced and variant == 'cost':
        variant = 'cem'
    segments = 0 if lean else int(rng.choice([0, 0, 2]))
    rc = 1 if lean else int(rng.choice([0, 0, 1, 2]))
    box, low, high = hp.random_action_bounds(rng, A)

    def want(name):
        if name in forced:
            return True
        if name == 'budget' and (variant != 'safe' or 'tail' in chosen):
            return False
        if name == 'tail' and (variant == 'cost' or everything == 'safe'):
            return False                                                        # (the safe "everything" handle takes the budget instead)
        return bool(rng.random() < (1.0 if everything else 0.3))
    chosen = set()
    for name in BATCH_OPTIONS:
        if want(name):
            chosen.add(name)
    tail_m = int(rng.integers(1, P + 1)) if 'tail' in chosen else 0
    cost_m = int(rng.integers(1, P + 1)) if 'budget' in chosen else 0
    budget = float(rng.choice([0.0, 0.5, 1.0, 2.0])) if cost_m else float('inf')
    tau = float(rng.choice([0.1, 0.5, 2.0])) if 'softmax' in chosen else 0.0
    noise = (('powerlaw', float(rng.choice([0.5, 2.0]))) if rng.random() < 0.5 else ('ar1', float(rng.choice([0.5, 0.9])))) if 'mixed' in chosen else None
    keep = cp.Keep(int(rng.integers(1, min(k, 4) + 1)), False, 1) if 'carry' in chosen else None
    warm = None
    if 'warm' in chosen:
        warm = cp.Warm(1 if stagger else int(rng.integers(1, H)), str(rng.choice(['box', 'repeat'])),
                       'keep' if stagger else str(rng.choice(['reset', 'keep'])), float(rng.choice([0.0, 0.25])))
    opt = cp.NOTHING._replace(tail_m=tail_m, cost_m=cost_m, budget=budget, tau=tau, noise=noise, keep=keep, readout='track' in chosen, warm=warm)
    smoothing = float(rng.choice([0.0, 0.1] if stagger else [0.0, 0.1, 0.5]))
    frac = STAGGER_FRACTION if stagger else float(rng.choice(THR_FRACTIONS))
    off = (not stagger) and bool(rng.random() < 0.8)                            # "about half" of all cases, the nine above included
    thr = -1.0 if off else float(F(frac * float(np.mean(hp.o.sampling_params(low, high)[3]))))
    case = cp.Case('batch_seed%d' % seed, O, A, H, N, P, E, k, I, units, depth, variant, 'fp32', smoothing, thr, float(rng.choice([0.0, 0.05])), box,
                   low, high, segments, rc, 900 + seed, opt)
    mb = int(rng.choice(MAX_BATCH))
    return case, mb


def _calls_plan(seed, case, mb):
    """The three calls of a case (the module docstring).  Drawn from a generator of its own, so that the shape draws do not move it."""
    rng = np.random.default_rng(81000 + seed)
    pb = cp.problem(case)
    warm = case.opt.warm is not None
    n2 = int(rng.integers(1, mb))                                               # fewer problems: 1 .. max_batch - 1
    numbers = rng.choice(1 << 40, size=2 * mb + n2, replace=False).astype(np.uint64)     # distinct, some above 2^32 (batch_cases.calls)
    if not (numbers >> np.uint64(32)).any():
        numbers[0] |= np.uint64(1) << np.uint64(33)

    def perm():
        while True:
            p = rng.permutation(mb)
            if mb == 1 or not np.array_equal(p, np.arange(mb)):
                return tuple(int(x) for x in p)
    p2, p3 = perm(), perm()
    while mb > 2 and p3 == p2:
        p3 = perm()
    sizes = (mb, n2, mb)
    slots = (None, p2[:n2], p3) if warm else (None, None, None)
    reset = (None, None, int(rng.integers(0, mb))) if warm else (None, None, None)
    calls, at = [], 0
    for j, n in enumerate(sizes):
        st = (pb['state'][None].astype(F) + rng.normal(0.0, STATE_SPREAD, (n, case.O)).astype(F)).astype(F)
        calls.append(Call(n, slots[j], reset[j], st, numbers[at:at + n].copy()))
        at += n
    return CallsPlan(bool(seed % 2), (1 << 33) + 17 * seed, tuple(calls))


def batch_case_for(seed):
    """(case, max_batch, calls_plan) of a seed: deterministic, drawn again until `batch_admitted` holds and the forced options are on."""
    seed = int(seed)
    j = seed % N_SEEDS                                                    # (CEM_FUZZ_SCALE: later rounds force the same pairs on other shapes)
    forced = frozenset(PAIRS[j]) if j < len(PAIRS) else frozenset()
    everything = EVERYTHING[j - len(PAIRS)] if j >= len(PAIRS) else None
    full = {'cem': 6, 'safe': 6, 'cost': 5}
    rng = np.random.default_rng(80000 + seed)
    for _ in range(1000):
        case, mb = _draw(seed, rng, forced, everything)
        if batch_admitted(case, mb) and forced <= cp.on(case) and (everything is None or len(cp.on(case)) == full[everything]):
            return case, mb, _calls_plan(seed, case, mb)
    raise AssertionError('no admitted batch case for seed %d' % seed)


def staggered():
    """{seed: call index} of tests/golden/batch_option_staggered.json: the calls whose problems' SINGLE-STATE plans end in different
    iterations, as recorded from a device run — in the batched launch of such a call some problems are done while others still run."""
    with open(STAGGERED_PATH) as f:
        rows = json.load(f)['staggered']
    return {int(r['seed']): int(r['call']) for r in rows}
