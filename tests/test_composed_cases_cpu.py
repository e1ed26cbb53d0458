"""tests/composed_cases.py on the host: the composed replay IS the per-option replays where one option is on, the generator covers what it
says it covers, and the composed reference notices the mistakes a shared host path could make (small mutants of its stages)."""
import dataclasses
import subprocess
import sys

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd.planner import inject_elites, mean_candidate, shift_distribution, track_best, warm_sigma_floor
from tests import composed_cases as cp
from tests import decay_cases as dc
from tests import elite_cases as ec
from tests import helpers as hp
from tests import readout_cases as rdc
from tests import warm_cases as wc

F, U = np.float32, np.uint32
SEEDS = range(cp.N_SEEDS)


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


def _same_result(got, want, keys, what):
    """got: one plan of cp.replay; want: (action, score, iterations, trace, ...) of a per-option oracle_plan."""
    _bits(got['action'], want[0], '%s: action' % what)
    assert F(got['score']).view(U) == F(want[1]).view(U) and got['iters'] == want[2] == len(want[3]), what
    for it, (g, w) in enumerate(zip(got['trace'], want[3])):
        for key in keys:
            if w[key] is None:
                assert g[key] is None, (what, it, key)
            else:
                _bits(g[key], w[key], '%s: iteration %d %s' % (what, it, key))


# ------------------------------------------------------------------------------------------------- the composed loop is the existing loops
def test_composed_cases_import_without_torch():
    r = subprocess.run([sys.executable, '-c', 'import sys; import tests.composed_cases; assert "torch" not in sys.modules'], cwd=hp.ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


@pytest.mark.parametrize('case,seed', ec.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in ec.ORACLE_CASES])
def test_with_carry_alone_replay_is_elite_cases_oracle_plan(case, seed):
    got = cp.replay(cp.from_elite(case), [hp.noise(ec.I, case.N, case.H, case.act, case.E, case.obs, seed=seed)])[0]
    _same_result(got, ec.oracle_plan(case, seed), ('actions', 'scores', 'elite', 'mu', 'sigma', 'store'), case.name)


@pytest.mark.parametrize('case,seed', dc.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in dc.ORACLE_CASES])
def test_with_a_schedule_alone_replay_is_decay_cases_oracle_plan(case, seed):
    noise = [hp.noise(dc.I, case.N, case.H, case.act, case.P, case.obs, seed=seed)]
    for with_mean in ((False, True) if case.name == 'lean' else (False,)):
        got = cp.replay(cp.from_decay(case, with_mean), noise)[0]
        _same_result(got, dc.oracle_plan(case, seed, with_mean=with_mean), ('actions', 'scores', 'elite', 'mu', 'sigma'),
                     '%s mean %s' % (case.name, with_mean))


@pytest.mark.parametrize('case,seed', rdc.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in rdc.ORACLE_CASES])
def test_with_the_readout_alone_replay_is_readout_cases_oracle_plan(case, seed):
    got = cp.replay(cp.from_readout(case), [hp.noise(rdc.I, case.N, case.H, case.act, case.P, case.obs, seed=seed)])[0]
    want = rdc.oracle_plan(case, seed)
    _same_result(got, want, ('actions', 'scores', 'elite', 'before', 'ret', 'costs'), case.name)
    for f in want[4]._fields:
        _bits(np.asarray(getattr(got['block'], f)), np.asarray(getattr(want[4], f)), '%s: block.%s' % (case.name, f))


WARM_BASE = dc.BY_NAME['ragged']                                                  # obs 10 / act 5, N 64, P = E = 5, H 5


@pytest.mark.parametrize('warm', [cp.Warm(1, 'box', 'reset', 0.0), cp.Warm(2, 'repeat', 'keep', 0.25)], ids=['pets', 'repeat_keep'])
def test_with_warm_start_alone_the_second_plan_is_warm_cases_oracle_plan(warm):
    """warm_cases.oracle_plan from warm_cases.shift (the independent, index-by-index restatement) of the first plan's last mu / sigma."""
    case = cp._from(WARM_BASE, WARM_BASE.P, dc.I, 0.01, cp.NOTHING._replace(warm=warm))
    noises = cp.noise_for(case, 3)
    first, second = cp.replay(case, noises)
    ref = cp.Reference(case)
    _bits(first['action'], o.do_generate_action(ref.pb['state'], ref.pb['weights'], ref.pb['inputs_min'], ref.pb['inputs_max'], ref.pb['low'],
                                                ref.pb['high'], *noises[0], ref.ocfg, ref.pb['scorer'])[0], 'the first plan is cold')
    mu0, sg0 = wc.box(ref.pb, case.H)
    m, g = wc.shift(first['mu'], first['sigma'], mu0[0], sg0[0], warm.shift, 1 if warm.tail == 'repeat' else 0, 1 if warm.sigma == 'keep' else 0,
                    warm_sigma_floor(ref.pcfg, warm.floor_frac))
    assert not np.array_equal(m, mu0)
    ra, rs, rit, rmu, rsg, rel = wc.oracle_plan(ref.pb['state'], ref.pb, ref.ocfg, noises[1], m, g)
    _bits(second['action'], ra, 'action')
    assert F(second['score']).view(U) == F(rs).view(U) and second['iters'] == rit
    _bits(second['mu'], rmu, 'mu'); _bits(second['sigma'], rsg, 'sigma')
    for it, el in enumerate(rel):
        _bits(np.sort(second['trace'][it]['elite']), el, 'iteration %d: elite set' % it)


def test_with_nothing_on_replay_is_do_generate_action():
    for base in (dc.BY_NAME['ragged'], dc.BY_NAME['two_blocks_safe']):
        case = cp._from(base, base.P, dc.I, 0.01, cp.NOTHING)
        assert cp.on(case) == frozenset()
        noise = hp.noise(dc.I, case.N, case.H, case.A, case.P, case.O, seed=4)
        ref, trace = cp.Reference(case), []
        want = o.do_generate_action(ref.pb['state'], ref.pb['weights'], ref.pb['inputs_min'], ref.pb['inputs_max'], ref.pb['low'], ref.pb['high'],
                                    *noise, ref.ocfg, ref.pb['scorer'], trace=trace)
        _same_result(cp.replay(case, [noise])[0], want + (trace,), ('actions', 'scores', 'elite', 'mu', 'sigma'), base.name)


# ------------------------------------------------------------------------------------------------- the generator
def _fingerprint(x):
    """A case as nested tuples, arrays by their bytes."""
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if dataclasses.is_dataclass(x):
        return tuple((f.name, _fingerprint(getattr(x, f.name))) for f in dataclasses.fields(x))
    if isinstance(x, tuple):
        return tuple(_fingerprint(v) for v in x)
    return x


def test_the_generator_covers_what_it_says():
    cases = [cp.case_for(s) for s in SEEDS]
    assert all(cp.admitted(c) for c in cases)
    assert len(cp.PAIRS) == 44 and ('tail', 'budget') not in cp.PAIRS
    for s, pair in enumerate(cp.PAIRS):
        assert set(pair) <= cp.on(cases[s]), (s, pair, cp.on(cases[s]))
    for name in cp.OPTIONS:
        assert sum(name in cp.on(c) for c in cases) >= 8, name
    assert {c.variant for c in cases} == {'cem', 'safe', 'cost'} and {c.precision for c in cases} == {'fp32', 'bf16x3', 'bf16'}
    ragged = [c for c in cases if any(n % 16 for n in cp.populations(c)) and c.opt.schedule is not None]
    to_k = [c for c in cases if c.opt.schedule is not None and c.opt.schedule[-1] == c.k]
    lean = [c for c in cases if cp.lean_eligible(c)]
    assert len(ragged) >= 4 and len(to_k) >= 2 and len(lean) >= 4, (len(ragged), len(to_k), len(lean))
    # a lean-eligible handle that leaves the lean path and comes back, and one that never leaves it
    assert any(any(cp.generic_forced(c, it) for it in range(c.I)) and not all(cp.generic_forced(c, it) for it in range(c.I)) for c in lean)
    assert any(not any(cp.generic_forced(c, it) for it in range(c.I)) for c in lean)
    # the four "everything" handles
    for s, kind in zip(range(44, 48), cp.EVERYTHING):
        c = cases[s]
        assert cp.on(c) == set(cp.OPTIONS) - ({'budget'} if kind in ('cem', 'bf16') else {'tail'} if kind == 'safe' else {'tail', 'budget'}), (s, cp.on(c))
        assert c.variant == ('cem' if kind == 'bf16' else kind) and c.precision == ('bf16' if kind == 'bf16' else 'fp32')
        assert c.opt.keep.across
    # the shapes stay where the issue puts them
    for c in cases:
        assert 24 <= c.N <= 96 and 2 <= c.H <= 6 and 2 <= c.I <= 4 and 1 <= c.A <= 6 and c.O in (9, 12, 31, 60, 70) and 1 <= c.E <= 4 and c.P <= 6
        assert c.units in (32, 64, 160) and c.segments in (0, 2)
    assert {c.units for c in cases} == {32, 64, 160} and {c.segments for c in cases} == {0, 2}
    assert {(c.O + c.A + 3) // 4 - c.O // 4 for c in cases} >= {1, 2}                  # one and two action quads (decay_cases.pad_layout)
    assert any(c.opt.keep is not None and c.opt.keep.across and c.opt.warm is not None for c in cases)
    assert any(c.opt.keep is not None and c.opt.mean and c.opt.schedule is not None for c in cases)


def test_a_seed_is_the_same_case_in_two_fresh_calls():
    for s in SEEDS:
        assert _fingerprint(cp.case_for(s)) == _fingerprint(cp.case_for(s)), s
    r = subprocess.run([sys.executable, '-c', 'from tests import composed_cases as cp; print(cp.case_for(7)._replace(opt=None, low=None, high=None))'],
                       cwd=hp.ROOT, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == str(cp.case_for(7)._replace(opt=None, low=None, high=None)), r.stderr[-2000:]


def test_admitted_refuses_what_admit_refuses():
    base = cp.case_for(0)
    c = base._replace(variant='safe', opt=cp.NOTHING._replace(tail_m=1, cost_m=1, budget=1.0))
    assert not cp.admitted(c) and cp.admitted(c._replace(opt=c.opt._replace(tail_m=0)))
    assert not cp.admitted(c._replace(variant='cem', opt=c.opt._replace(tail_m=0)))                     # the budget needs 'safe'
    assert not cp.admitted(base._replace(variant='cost', opt=cp.NOTHING._replace(tail_m=1)))
    n, k = base.N, base.k
    sched = (n,) * (base.I - 1) + (k,)
    plain = base._replace(opt=cp.NOTHING._replace(schedule=sched if (base.P * k) % base.E == 0 else None))
    assert cp.admitted(plain)
    assert not cp.admitted(plain._replace(opt=plain.opt._replace(keep=cp.Keep(k, False, 1))))            # m < n[it] for every it
    assert not cp.admitted(base._replace(opt=cp.NOTHING._replace(keep=cp.Keep(base.k, False, 1), mean=True, schedule=(n,) * (base.I - 1) + (k + 1,))))
    assert not cp.admitted(base._replace(H=1, opt=cp.NOTHING._replace(warm=cp.Warm(1, 'box', 'reset', 0.0))))
    assert not cp.admitted(base._replace(H=1, opt=cp.NOTHING._replace(keep=cp.Keep(1, True, 1))))
    assert cp.admitted(base._replace(H=1, opt=cp.NOTHING._replace(keep=cp.Keep(1, False, 1))))
    assert not cp.admitted(base._replace(opt=cp.NOTHING._replace(schedule=(n,) * (base.I - 1) + (k - 1,))))
    assert not cp.admitted(base._replace(opt=cp.NOTHING._replace(schedule=(n + 1,) + (n,) * (base.I - 1))))
    assert not cp.admitted(base._replace(P=3, E=2, N=33, k=2, opt=cp.NOTHING))                            # P n % E


# ------------------------------------------------------------------------------------------------- the reference has teeth
class InjectShiftAtLaterIterations(cp.Reference):
    """The handle's shift applied by every inject, not only by a later plan's first."""

    def candidates(self, it, mu, sigma, eps_it, store, plan_index):
        n, k = self.n[it], self.opt.keep
        acts = o.sample_actions(mu, sigma, self.lb, self.ub, np.asarray(eps_it, F)[:n]).astype(F)
        if k is not None and store is not None and (it > 0 or (plan_index > 0 and k.across)):
            acts = inject_elites(acts, store, k.m, k.shift)
        if self.opt.mean and it == self.case.I - 1:
            acts = mean_candidate(acts, mu, self.lb, self.ub)
        return acts


class InjectAfterTheMeanRow(cp.Reference):
    def candidates(self, it, mu, sigma, eps_it, store, plan_index):
        n, k = self.n[it], self.opt.keep
        acts = o.sample_actions(mu, sigma, self.lb, self.ub, np.asarray(eps_it, F)[:n]).astype(F)
        if self.opt.mean and it == self.case.I - 1:
            acts = mean_candidate(acts, mu, self.lb, self.ub)
        if k is not None and store is not None and (it > 0 or (plan_index > 0 and k.across)):
            acts = inject_elites(acts, store, k.m, 0 if it > 0 else k.shift)
        return acts


class KeepReadsThePreviousScores(cp.Reference):
    """The keep launched before the iteration's scores are final: it ranks the elites by what the previous iteration left in `scores`."""
    stale = None

    def keep(self, scores, elite, actions):
        old, self.stale = self.stale, np.array(scores, F)
        if old is not None:
            seen = np.array(scores, F)
            seen[:min(old.size, seen.size)] = old[:seen.size]
            scores = seen
        return super().keep(scores, elite, actions)


class TrackerReadsWithTheHandlesWidth(cp.Reference):
    """The tracker given the handle's N as the width of `ret` and the cost bytes, not n[it]."""

    def track(self, block, it, iters, best_score, scores, elite, actions, ret, costs):
        c, n = self.case, self.n[it]
        flat = np.zeros(c.P * c.N, F); flat[:c.P * n] = np.asarray(ret, F).reshape(-1)
        cb = None
        if self.has_costs:
            cb = np.zeros(c.H * c.P * c.N, np.uint8); cb[:c.H * c.P * n] = np.asarray(costs, np.uint8).reshape(-1)
        sc = np.full(c.N, -np.inf, F); sc[:n] = scores
        act = np.zeros((c.N, c.H, c.A), F); act[:n] = actions
        return track_best(block, it, iters, best_score, sc, elite, act, flat, cb, n=c.N)


class WarmShiftOnTheFirstPlan(cp.Reference):
    """The shift applied whether or not the carry is valid (an invalid carry reads as zeros)."""

    def init(self, plan_index, carry, store):
        mu, sigma, st = super().init(plan_index, carry, store)
        w = self.opt.warm
        if w is not None and plan_index == 0:
            mu, sigma = shift_distribution(carry[0], carry[1], self.mu0, self.sg0, w.shift, 1 if w.tail == 'repeat' else 0,
                                           1 if w.sigma == 'keep' else 0, warm_sigma_floor(self.pcfg, w.floor_frac))
        return mu, sigma, st


def _differs(a, b):
    for pa, pb in zip(a, b):
        if pa['iters'] != pb['iters'] or not np.array_equal(pa['action'].view(U), pb['action'].view(U)) or F(pa['score']).view(U) != F(pb['score']).view(U):
            return True
        if any(not np.array_equal(np.asarray(x).view(U) if np.asarray(x).dtype == F else np.asarray(x), np.asarray(y).view(U) if np.asarray(y).dtype == F else np.asarray(y))
               for x, y in zip(pa['block'], pb['block'])):
            return True
        for ta, tb in zip(pa['trace'], pb['trace']):
            if not np.array_equal(ta['actions'].view(U), tb['actions'].view(U)) or not np.array_equal(ta['scores'].view(U), tb['scores'].view(U)):
                return True
            if ta['store'] is not None and not np.array_equal(ta['store'].view(U), tb['store'].view(U)):
                return True
    return False


_REPLAYS = {}


def _replayed(seed):
    if seed not in _REPLAYS:
        case = cp.case_for(seed)
        _REPLAYS[seed] = (case, cp.noise_for(case, seed), cp.replay(case, cp.noise_for(case, seed)))
    return _REPLAYS[seed]


@pytest.mark.parametrize('mutant,needs', [(InjectShiftAtLaterIterations, {'carry'}), (KeepReadsThePreviousScores, {'carry'}),
                                          (TrackerReadsWithTheHandlesWidth, {'track', 'sched'}), (WarmShiftOnTheFirstPlan, {'warm'})],
                         ids=lambda m: getattr(m, '__name__', ''))
def test_the_composed_reference_has_teeth(mutant, needs):
    """Each mistake changes what `replay` returns (actions, scores, kept elites, the read-out block or the result) on at least one seed."""
    caught = []
    for s in SEEDS:
        case = cp.case_for(s)
        if not needs <= cp.on(case):
            continue
        case, noises, want = _replayed(s)
        if _differs(cp.replay(case, noises, ref=mutant(case)), want):
            caught.append(s)
            if len(caught) >= 2:
                break
    assert caught, mutant.__name__


def test_inject_and_mean_row_commute_on_every_admitted_case():
    """admit() keeps the inject's rows (n < n_keep) and the mean candidate's row (n[last] - 1) apart — n_keep < n[last] - 1 — so on an
    admitted combination the ORDER of the two launches cannot be observed: the mutant that swaps them returns what `replay` returns, on
    every seed that has both on.  (What the order could change is ruled out by the option rule, which tests/golden/option_statuses.json
    pins; a mutant that breaks the RULE is caught: the two kernels then write the same row.)"""
    both = [s for s in SEEDS if {'carry', 'mean'} <= cp.on(cp.case_for(s))]
    assert len(both) >= 3
    for s in both[:4]:
        case, noises, want = _replayed(s)
        assert not _differs(cp.replay(case, noises, ref=InjectAfterTheMeanRow(case)), want), s
