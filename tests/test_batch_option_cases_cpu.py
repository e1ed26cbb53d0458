"""tests/batch_option_cases.py on the host: the table behind tests/test_gpu_batch_option_fuzz.py is what it says — every case is one a
batch handle admits (so a device failure there is never a refusal in disguise), the forced pairs are on, the shapes reach the corners the
device test is meant to cover, and tests/golden/batch_option_staggered.json lists enough launches in which some problems are done while
others still run.  No compute calls."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np

from ethz_safe_learning_amd.planner import to_c_config
from tests import batch_option_cases as bo
from tests import composed_cases as cp
from tests import helpers as hp
from tests.test_composed_cases_cpu import _fingerprint

HUNT_SCALE = 3                                        # the draws of a CEM_FUZZ_SCALE=3 run are checked too
SEEDS = range(bo.N_SEEDS)


def _cases(scale=1):
    return [bo.batch_case_for(s) for s in range(bo.N_SEEDS * scale)]


def test_batch_option_cases_import_without_torch():
    r = subprocess.run([sys.executable, '-c', 'import sys; import tests.batch_option_cases; assert "torch" not in sys.modules'], cwd=hp.ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def test_every_case_is_admitted_by_a_batch_handle(built_lib):
    for case, mb, plan in _cases(HUNT_SCALE):
        assert bo.batch_admitted(case, mb), case
        # ... and by the library's own validate_batch, on the batch side's configuration (never segmented) and the single side's
        pb = cp.problem(case)
        for kw in (dict(rollout_segments=0), dict()):
            cc = to_c_config(hp.configs(pb, **cp.config_kwargs(case, use_graph=plan.use_graph, **kw))[1])
            assert built_lib.cem_workspace_bytes(C.byref(cc)) > 0, case
        assert built_lib.cem_batch_workspace_bytes(C.byref(cc), mb) > 0, case


def test_the_table_covers_what_it_says():
    table = _cases()
    cases = [c for c, _, _ in table]
    assert bo.N_SEEDS == 23 and len(bo.PAIRS) == 20 and ('tail', 'budget') not in bo.PAIRS
    assert {frozenset(p) for p in bo.PAIRS} == {frozenset(p) for p in cp.PAIRS if set(p) <= set(bo.BATCH_OPTIONS)}
    for s, pair in enumerate(bo.PAIRS):
        assert set(pair) <= cp.on(cases[s]), (s, pair, cp.on(cases[s]))
    for name in bo.BATCH_OPTIONS:
        assert sum(name in cp.on(c) for c in cases) >= 6, name
    # the three "everything" handles
    for s, kind in zip(range(20, 23), bo.EVERYTHING):
        want = set(bo.BATCH_OPTIONS) - ({'budget'} if kind == 'cem' else {'tail'} if kind == 'safe' else {'tail', 'budget'})
        assert cp.on(cases[s]) == want and cases[s].variant == kind, (s, cp.on(cases[s]))
    # never: a schedule, the mean candidate, a task, across-plans carry, another precision, the wide family
    for c in cases:
        assert cp.on(c) <= set(bo.BATCH_OPTIONS) and c.precision == 'fp32' and c.units in bo.UNITS
        assert c.opt.keep is None or (not c.opt.keep.across)
    assert {c.variant for c in cases} == {'cem', 'safe', 'cost'}
    assert {p.use_graph for _, _, p in table} == {True, False} and abs(sum(p.use_graph for _, _, p in table) - len(table) / 2) <= 1
    assert {mb for _, mb, _ in table} == set(bo.MAX_BATCH)
    # both membership kinds: whole particles per member, and members that split a particle
    assert any(c.P % c.E == 0 for c in cases) and any(c.P % c.E for c in cases)
    # the lean-eligible shapes: every fourth seed of the pairs; some single side rolls out lean, some is forced off it by its options
    lean = [s for s in SEEDS if cp.lean_eligible(cases[s])]
    assert set(lean) >= {s for s in range(20) if s % 4 == 0} and all(cases[s].A == 2 and cases[s].O == 12 for s in range(0, 20, 4)), lean
    assert any(not any(cp.generic_forced(cases[s], it) for it in range(cases[s].I)) for s in lean)
    assert any(cp.generic_forced(cases[s], 0) for s in lean)
    # the shapes stay where the issue puts them
    for c in cases:
        assert 24 <= c.N <= 96 and 2 <= c.H <= 6 and 2 <= c.I <= 4 and 1 <= c.E <= 4 and c.P <= 6 and 2 <= c.depth <= 4, c
        assert c.O in bo.OBS_DIMS and c.A in (1, 2, 3, 5, 7, 8) and c.rc in (0, 1, 2) and c.segments in (0, 2), c
    assert any(c.N % 16 for c in cases) and any(c.N % 16 == 0 for c in cases)
    assert sum(c.A == 2 for c in cases) <= len(cases) / 4
    assert sum(c.A >= 5 for c in cases) >= 5                                       # two action quads
    assert {c.A for c in cases} == {1, 2, 3, 5, 7, 8}
    assert {c.rc for c in cases} == {0, 1, 2} and {c.segments for c in cases} == {0, 2}
    assert len({c.units for c in cases}) >= 3
    # the threshold: off on about half of the cases
    off = sum(c.thr < 0 for c in cases)
    assert 0.35 * len(cases) <= off <= 0.65 * len(cases), off


def test_the_calls_are_what_the_device_test_expects():
    for seed, (case, mb, plan) in enumerate(_cases(HUNT_SCALE)):
        a, b, c = plan.calls
        assert (a.n, c.n) == (mb, mb) and 1 <= b.n < mb, (seed, a.n, b.n, c.n)
        if case.opt.warm is not None:
            assert a.slots is None and a.reset is None and b.reset is None
            assert len(set(b.slots)) == b.n and set(b.slots) <= set(range(mb))
            assert sorted(c.slots) == list(range(mb)) and c.slots != tuple(range(mb)) and 0 <= c.reset < mb
            assert mb == 2 or c.slots != bo.slot_rows(a, mb)
        else:
            assert all(x.slots is None and x.reset is None for x in plan.calls)
        numbers = np.concatenate([x.calls for x in plan.calls])
        assert numbers.dtype == np.uint64 and len(set(numbers.tolist())) == numbers.size and (numbers >> np.uint64(32)).any()
        states = np.concatenate([x.states for x in plan.calls])
        assert states.dtype == np.float32 and states.shape == (numbers.size, case.O)
        assert len({s.tobytes() for s in states}) == len(states)                     # distinct per slot and per call
        assert float(np.std(states - cp.problem(case)['state'])) > 0.25             # ... and spread widely
        assert plan.plan_seed >> 32                                                  # (the seed's high word too)
    # the warm cases permute: some call-2 map is no prefix of the identity
    assert any(p.calls[1].slots is not None and p.calls[1].slots != tuple(range(p.calls[1].n)) for _, _, p in _cases())


def test_a_seed_is_the_same_case_in_two_fresh_processes():
    def key(seed):
        case, mb, plan = bo.batch_case_for(seed)
        return _fingerprint((tuple(case), mb, plan.use_graph, plan.plan_seed, tuple(tuple(c) for c in plan.calls)))
    for s in SEEDS:
        assert key(s) == key(s), s
    code = ('import hashlib; from tests import batch_option_cases as bo; from tests.test_batch_option_cases_cpu import _digest; '
            'print(_digest(7), _digest(21))')
    outs = [subprocess.run([sys.executable, '-c', code], cwd=hp.ROOT, capture_output=True, text=True) for _ in range(2)]
    assert all(r.returncode == 0 for r in outs), outs[0].stderr[-2000:]
    assert outs[0].stdout == outs[1].stdout == '%s %s\n' % (_digest(7), _digest(21))


def _digest(seed):
    import hashlib
    case, mb, plan = bo.batch_case_for(seed)
    return hashlib.sha256(repr(_fingerprint((tuple(case), mb, plan.use_graph, plan.plan_seed, tuple(tuple(c) for c in plan.calls)))).encode()).hexdigest()


def test_batch_admitted_refuses_what_a_batch_handle_refuses():
    case, mb, _ = bo.batch_case_for(2)                                               # tail x carry, N 41
    assert bo.batch_admitted(case, mb) and case.opt.keep is not None
    n = tuple([case.N] * (case.I - 1) + [case.N - 1])
    sched = case._replace(opt=case.opt._replace(schedule=n))
    assert cp.admitted(sched) and not bo.batch_admitted(sched, mb)                   # a schedule
    mean = case._replace(opt=case.opt._replace(mean=True))
    assert cp.admitted(mean) and not bo.batch_admitted(mean, mb)                     # the mean candidate
    from tests import task_cases as tc
    task = case._replace(opt=case.opt._replace(task=tc.task_for(case.O, case.A, 1, False)))
    assert cp.admitted(task) and not bo.batch_admitted(task, mb)                     # a task
    across = case._replace(opt=case.opt._replace(keep=case.opt.keep._replace(across=True)))
    assert cp.admitted(across) and not bo.batch_admitted(across, mb)                 # across-plans carry
    assert not bo.batch_admitted(case._replace(precision='bf16'), mb)
    assert not bo.batch_admitted(case._replace(precision='bf16x3'), mb)
    assert cp.admitted(case._replace(units=160)) and not bo.batch_admitted(case._replace(units=160), mb)
    assert not bo.batch_admitted(case, 0) and not bo.batch_admitted(case, bo.BATCH_CAP + 1) and bo.batch_admitted(case, bo.BATCH_CAP)
    # ... and what composed_cases.admitted refuses
    assert not bo.batch_admitted(case._replace(variant='cost'), mb)                  # the tail has no returns to read there


def test_the_staggered_list_is_well_formed_and_large_enough():
    with open(bo.STAGGERED_PATH) as f:
        doc = json.load(f)
    assert set(doc) == {'staggered'}
    rows = doc['staggered']
    assert all(set(r) == {'seed', 'call'} and type(r['seed']) is int and type(r['call']) is int for r in rows), rows
    seeds = [r['seed'] for r in rows]
    assert seeds == sorted(set(seeds)) and all(0 <= s < bo.N_SEEDS for s in seeds), seeds
    assert all(0 <= r['call'] < 3 for r in rows)
    assert len(seeds) >= 6, seeds
    listed = bo.staggered()
    for s, j in listed.items():
        case, mb, plan = bo.batch_case_for(s)
        assert case.thr > 0 and plan.calls[j].n >= 2, (s, j)                         # a launch that CAN stagger
    for name in ('carry', 'track', 'softmax', 'mixed', 'warm'):
        assert any(name in cp.on(bo.batch_case_for(s)[0]) for s in listed), name
