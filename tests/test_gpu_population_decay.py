"""Per-iteration population sizes and the mean candidate (cem_planner_set_population_schedule, cem_planner_set_mean_candidate;
DESIGN.md 4.13) on the device.

The contract has an exact reference that costs nothing: iteration `it` of a scheduled plan IS iteration `it` of a handle created with
n_samples = n[it] on the same mu / sigma, seed and call.  So the stepwise form is held bit for bit, launch by launch, to such handles
over tests/decay_cases.py, with everything beyond the leading n[it] entries poisoned (1, 2); everything else — the oracle's replay, the
plan forms, early stop, off is off, the other settings, the mean candidate, refusals, policies — hangs off that."""
import ctypes

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd import BatchCemPlanner, _capi
from ethz_safe_learning_amd.planner import (inject_elites, keep_elites, mean_candidate, mix_noise, population_schedule,
                                            powerlaw_mixing, softmax_refit)
from tests import decay_cases as dc
from tests import helpers as hp

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
SCORE_ATOL = 2e-5                        # tests/test_gpu_parity.py FULL_SIZE_ATOL, tests/test_gpu_whole_plan.py SCORE_ATOL
SEED, CALL = dc.PLAN_SEED, dc.PLAN_CALL
I = dc.I
IDS = [c.name for c in dc.CASES]


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


def _planner(case, schedule='case', mean=False, **over):
    """A handle of the case; schedule 'case': the case's own, None: never set, else the list to set."""
    _torch()
    pb = dc.problem(case)
    _, pcfg = hp.configs(pb, **dc.config_kwargs(case, **over))
    pl = hp.make_planner(pb, pcfg)
    if schedule is not None:
        pl.set_population_schedule(list(case.schedule) if schedule == 'case' else schedule)
    if mean:
        pl.set_mean_candidate(True)
    return pb, pl


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except _capi.CemError as e:
        return e.status
    return 0


Arrays = hp.Arrays                       # (tests/test_gpu_option_fuzz.py poisons with the same helper)


def _plain(case, n, cache):
    """A handle created with n_samples = n (never scheduled), 'explicit' initial distribution; one per population and case."""
    if n not in cache:
        pb, pl = _planner(case, schedule=None, N=n)
        pl.set_init_mode('explicit')
        cache[n] = pl
    return cache[n]


def _plain_iteration(plain, pb, ms, it, seed=SEED, call=CALL):
    """Iteration `it` of a plain handle begun from mu / sigma ms: -> dict of what its rollout and select leave."""
    plain.set_initial_distribution(ms[0], ms[1])
    plain.plan_begin(pb['state'], seed=seed, call=call)
    plain.plan_rollout(it)
    out = dict(actions=_np(plain.actions()), scores=_np(plain.scores_local()), returns=_np(plain.returns()), costs=_np(plain.costs()))
    plain.plan_select(it)
    out.update(elite=_np(plain.elite_idx()), mu_sigma=_np(plain.mu_sigma()))
    plain.plan_end()
    return out


def _plain_pad(plain, case, n):
    pf, _ = dc.pad_layout(case)
    off = dc.pad_offset(plain.layout.actions, case._replace(N=n))
    plain.synchronize()
    return _np(plain._ws_view[off:off + n * case.H * pf * 4].view(_torch().float32))


# ------------------------------------------------------------------------------------------------- 1, 2: every iteration is the plain handle's
@pytest.mark.parametrize('case', dc.CASES, ids=IDS)
def test_each_iteration_is_the_plain_handles_and_nothing_beyond_it_is_touched(case):
    """Teeth.  Stepwise on Philox noise, everything beyond the leading n[it] entries poisoned in front of every launch: actions, the
    padded actions, scores, returns and costs, then elite indices and mu / sigma are the bits of a handle created with n_samples = n[it]
    and begun from the same mu / sigma; the poison is intact; iteration_plan reports that handle's plan."""
    pb, pl = _planner(case)
    assert pl.population_schedule() == (list(case.schedule), True)
    arr, plains = Arrays(pl, case), {}
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(I):
        n = case.schedule[it]
        plain = _plain(case, n, plains)
        ms = _np(pl.mu_sigma())
        want = _plain_iteration(plain, pb, ms, it)
        # the plain handle's padded actions as its rollout left them (its select does not touch them)
        want_pad = _plain_pad(plain, case, n)
        arr.poison(n)
        pl.plan_rollout(it)
        arr.check(n, 'iteration %d rollout' % it)
        _bits(arr.get('actions', n), want['actions'].reshape(-1), 'iteration %d: actions' % it)
        _bits(arr.get('act_pad', n), want_pad, 'iteration %d: act_pad' % it)
        _bits(arr.get('scores', n), want['scores'], 'iteration %d: scores' % it)
        _bits(arr.get('returns', n), want['returns'].reshape(-1), 'iteration %d: returns' % it)
        if case.variant != 'cem':
            _bits(arr.get('costs', n, np.uint8), want['costs'].reshape(-1), 'iteration %d: cost bytes' % it)
        arr.poison(n)
        pl.plan_select(it)
        arr.check(n, 'iteration %d select' % it)
        _bits(_np(pl.elite_idx()), want['elite'], 'iteration %d: elite indices' % it)
        _bits(_np(pl.mu_sigma()), want['mu_sigma'], 'iteration %d: mu / sigma' % it)
        assert _np(pl.elite_idx()).max() < n
        ip = pl.iteration_plan(it)
        rc, tiles = plain.tiles()
        assert (ip['n_samples'], ip['chunks_per_tile'], ip['n_tiles']) == (n, rc, len(tiles)), (it, ip)
        assert ip['n_segments'] == plain.segments()[0] and ip['launches'] == plain.launches_per_iteration(), (it, ip)
        assert ip['rollout_path'] == plain.rollout_path() == plain.iteration_plan(0)['rollout_path'], (it, ip)
        assert ip == dict(plain.iteration_plan(it), n_samples=n)
        if case.lean:
            assert ip['rollout_path'] == 'lean'
    a, s, n_it = pl.plan_end()
    assert n_it == I and np.isfinite(s) and np.isfinite(a).all()
    for p in list(plains.values()) + [pl]:
        p.close()


# ------------------------------------------------------------------------------------------------- 3: the oracle's replay
@pytest.mark.parametrize('case,seed', dc.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in dc.ORACLE_CASES])
def test_whole_plan_against_the_oracle_replay(case, seed):
    """The fp32 oracle's replay per iteration with n[it] candidates on the same noise tensors, cut as the contract says.  The seeds keep the
    cut wider than dc.ORACLE_GAP in the oracle (tests/test_decay_cases_cpu.py), so the elite sets must be EQUAL."""
    pb, pl = _planner(case)
    ra, rs, rit, trace = dc.oracle_plan(case, seed)
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.P, case.obs, seed=seed)
    arr = Arrays(pl, case)
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    for it in range(I):
        n = case.schedule[it]
        pl.plan_rollout(it)
        acts, scores = arr.get('actions', n).reshape(n, case.H, case.act), arr.get('scores', n)
        np.testing.assert_allclose(acts, trace[it]['actions'], rtol=1e-5, atol=1e-6, err_msg='iteration %d: actions' % it)
        err = np.abs(scores - trace[it]['scores'])
        print('%s seed %d iteration %d: max score error %.3g' % (case.name, seed, it, err.max()))
        # (a `<=` of the objective may resolve differently within rounding and move a score by a whole unit: rare, and never on a cut)
        flipped = err > SCORE_ATOL + 6e-8 * np.abs(trace[it]['scores'])
        assert flipped.mean() <= 0.03 and (not flipped.any() or err[flipped].min() > 1e-3), 'iteration %d: %d scores off, by %.3g at least' % (
            it, flipped.sum(), err[flipped].min() if flipped.any() else 0.0)
        pl.plan_select(it)
        np.testing.assert_array_equal(np.sort(_np(pl.elite_idx())), np.sort(trace[it]['elite']), err_msg='iteration %d: elite set' % it)
        ms = _np(pl.mu_sigma())
        np.testing.assert_allclose(ms[0], trace[it]['mu'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(ms[1], trace[it]['sigma'], rtol=1e-5, atol=1e-6)
    a, s, n_it = pl.plan_end(eps_out=eo)
    assert n_it == rit == I
    np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-7)
    assert abs(s - rs) <= SCORE_ATOL
    r = pl.plan(pb['state'], eps_act=ea, eps_model=em, eps_out=eo)                # the same tensors through the whole-plan call
    _bits(r[0], a, 'the eager tensor-fed plan'); assert F(r[1]).view(U) == F(s).view(U)
    pl.close()


# ------------------------------------------------------------------------------------------------- 4: the plan forms agree; early stop
def _left(pl):
    return dict(mu_sigma=_np(pl.mu_sigma()), elite_idx=_np(pl.elite_idx()), actions=_np(pl.actions()), scores=_np(pl.scores_local()))


def _same_plan(got, want, left_got, left_want, what):
    _bits(got[0], want[0], '%s: action' % what)
    assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2], (what, got, want)
    for key in left_want:
        _bits(left_got[key], left_want[key], '%s: %s' % (what, key))


def _stepwise(pl, state, seed=SEED, call=CALL, iters=I):
    pl.plan_begin(state, seed=seed, call=call)
    for it in range(iters):
        pl.plan_rollout(it)
        pl.plan_select(it)
    return pl.plan_end()


def _zero_arrays(pl):
    """What a plan leaves beyond its last iteration's population depends on the handle's history: start the forms from the same bytes."""
    pl.synchronize()
    with pl.stream_context():
        pl.actions(sync=False).zero_(); pl.scores_local(sync=False).zero_()
    pl.synchronize()


@pytest.mark.parametrize('case', dc.CASES, ids=IDS)
def test_graph_eager_and_stepwise_plans_agree(case, mean=False):
    pb, ps = _planner(case, mean=mean)
    _zero_arrays(ps)
    want = _stepwise(ps, pb['state'])
    left = _left(ps)
    pb, pe = _planner(case, mean=mean)
    _zero_arrays(pe)
    _same_plan(pe.plan(pb['state'], seed=SEED, call=CALL), want, _left(pe), left, 'eager')
    assert pe.graph_status() == 'eager'
    pb, pg = _planner(case, mean=mean, use_graph=True)
    _zero_arrays(pg)
    for rep in range(2):                                                          # captured, then replayed
        _same_plan(pg.plan(pb['state'], seed=SEED, call=CALL), want, _left(pg), left, 'graph, plan %d' % rep)
        assert pg.graph_status() == 'graph'
    pt = None
    if case.name in ('lean', 'segments'):                                         # a timing handle launches eagerly, events around every launch
        pb, pt = _planner(case, mean=mean)
        _zero_arrays(pt)
        pt.set_timing(True)
        _same_plan(pt.plan(pb['state'], seed=SEED, call=CALL), want, _left(pt), left, 'timing')
        assert pt.last_timing()['rollout_launches'] == I
    for p in (ps, pe, pg, pt):
        if p is not None:
            p.close()


def test_mean_candidate_plan_forms_agree():
    test_graph_eager_and_stepwise_plans_agree(dc.BY_NAME['lean'], mean=True)
    test_graph_eager_and_stepwise_plans_agree(dc.BY_NAME['ragged'], mean=True)


def test_an_early_stop_leaves_the_later_iterations_arrays_untouched():
    case = dc.BY_NAME['grow']                                                     # iteration 2 would be narrower than iteration 1, wider than 0
    pb, pl = _planner(case)
    sig = []
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(I):
        pl.plan_rollout(it)
        pl.plan_select(it)
        sig.append(float(_np(pl.mu_sigma())[1].mean(dtype=F)))
    pl.plan_end()
    pl.close()
    assert sig[1] < sig[0], sig
    thr = 0.5 * (sig[0] + sig[1])                                                 # the select of iteration 1 stops the plan
    for mean in (False, True):
        pb, pl = _planner(case, thr=thr, mean=mean)
        pl.plan_begin(pb['state'], seed=SEED, call=CALL)
        for it in range(2):
            pl.plan_rollout(it)
            pl.plan_select(it)
        want = _left(pl)
        arr = Arrays(pl, case)
        arr.poison(0)                                                             # every byte of every per-candidate array
        pl.plan_rollout(2)                                                        # sampler, (mean candidate,) rollout, reduce, select: all leave at once
        pl.plan_select(2)
        arr.check(0, 'the iteration that did not run')
        got = _left(pl)
        for key in want:
            _bits(got[key], want[key], 'after the iteration that did not run: %s' % key)
        a, s, n_it = pl.plan_end()
        assert n_it == 2
        for use_graph in (False, True):
            pb, pw = _planner(case, thr=thr, mean=mean, use_graph=use_graph)
            r = pw.plan(pb['state'], seed=SEED, call=CALL)
            _bits(r[0], a, 'whole plan that stops early'); assert F(r[1]).view(U) == F(s).view(U) and r[2] == 2
            _bits(_np(pw.mu_sigma()), want['mu_sigma']); _bits(_np(pw.elite_idx()), want['elite_idx'])
            pw.close()
        pl.close()


# ------------------------------------------------------------------------------------------------- 5: off is off
def test_off_is_off_and_the_lean_path_stays():
    case = dc.BY_NAME['lean']
    pb, fresh = _planner(case, schedule=None, use_graph=True)
    want = fresh.plan(pb['state'], seed=SEED, call=CALL)
    left = _left(fresh)
    assert fresh.rollout_path() == 'lean' and fresh.launches_per_iteration() == 2
    assert fresh.population_schedule() == ([case.N] * I, False) and fresh.mean_candidate() is False
    base_plan = [fresh.iteration_plan(it) for it in range(I)]
    assert all(p == base_plan[0] and p['n_samples'] == case.N and p['launches'] == 2 and p['rollout_path'] == 'lean' for p in base_plan)

    def off_none(pl):
        pl.set_population_schedule(None)

    def off_all_n(pl):
        pl.set_population_schedule([case.N] * I)

    def off_set_unset(pl):
        pl.set_population_schedule(list(case.schedule))
        assert pl.population_schedule()[1] is True
        pl.plan(pb['state'], seed=SEED, call=CALL)
        pl.set_mean_candidate(True)
        assert pl.iteration_plan(I - 1)['rollout_path'] == 'generic'
        pl.set_mean_candidate(False)
        pl.set_population_schedule(None)

    for how in (off_none, off_all_n, off_set_unset):
        _, pl = _planner(case, schedule=None, use_graph=True)
        how(pl)
        assert pl.population_schedule() == ([case.N] * I, False), how.__name__
        assert [pl.iteration_plan(it) for it in range(I)] == base_plan and pl.rollout_path() == 'lean' and pl.launches_per_iteration() == 2
        got = pl.plan(pb['state'], seed=SEED, call=CALL)
        _same_plan(got, want, _left(pl), left, how.__name__)
        assert pl.graph_status() == 'graph'
        assert pl.lib.cem_workspace_bytes(ctypes.byref(pl.ccfg)) == fresh.lib.cem_workspace_bytes(ctypes.byref(fresh.ccfg))
        assert [getattr(pl.layout, f) for f, _ in pl.layout._fields_] == [getattr(fresh.layout, f) for f, _ in fresh.layout._fields_]
        pl.close()
    fresh.close()


# ------------------------------------------------------------------------------------------------- 6: together with the other settings
def test_with_keep_elites_launch_by_launch_and_across_plans():
    case = dc.BY_NAME['lean']
    m = 3
    pb, pl = _planner(case)
    pl.set_elite_carry(m, True, 1)
    assert all(pl.iteration_plan(it)['rollout_path'] == 'generic' for it in range(I))
    lb, ub, _, _ = o.sampling_params(pb['low'], pb['high'])
    arr = Arrays(pl, case)
    last_store = None
    for plan in range(2):
        ea = _np(pl.fill_noise(seed=SEED, call=CALL + plan)[0])
        pl.plan_begin(pb['state'], seed=SEED, call=CALL + plan)
        store = None
        for it in range(I):
            n = case.schedule[it]
            ms = _np(pl.mu_sigma())
            pl.plan_rollout(it)
            acts = arr.get('actions', n).reshape(n, case.H, case.act)
            drawn = o.sample_actions(ms[0], ms[1], lb, ub, ea[it][:n])            # (action noise is keyed on the candidate index alone)
            if it == 0 and plan == 0:
                _bits(acts, drawn, 'the first plan\'s first iteration: the plain sampler')
            elif it == 0:
                _bits(acts, inject_elites(drawn, last_store, m, 1), 'plan 1 iteration 0: the previous plan\'s store, shifted')
            else:
                _bits(acts, inject_elites(drawn, store, m, 0), 'plan %d iteration %d: inject_elites' % (plan, it))
            pl.plan_select(it)
            store, count = pl.elite_store()
            assert count == m
            _bits(store, keep_elites(arr.get('scores', n), _np(pl.elite_idx()), acts, m), 'plan %d iteration %d: keep_elites' % (plan, it))
        pl.plan_end()
        last_store = store
    pl.close()


def test_with_mixed_action_noise_the_slabs_stay_n_samples_wide():
    case = dc.BY_NAME['lean']
    pb, pl = _planner(case)
    pl.set_action_noise('powerlaw', 2.0)
    assert all(pl.iteration_plan(it)['rollout_path'] == 'generic' for it in range(I))
    lb, ub, _, _ = o.sampling_params(pb['low'], pb['high'])
    xi = _np(pl.fill_noise(seed=SEED, call=CALL)[0])                              # the white streams, [I, N, H, A]
    M = powerlaw_mixing(case.H, 2.0)
    arr = Arrays(pl, case)
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(I):
        n = case.schedule[it]
        ms = _np(pl.mu_sigma())
        pl.plan_rollout(it)
        eps = np.asarray(pl.action_noise_tensor())                                      # the handle's own tensor: all N rows of every slab filled
        assert eps.shape == (I, case.N, case.H, case.act)
        np.testing.assert_allclose(eps, mix_noise(M, xi), rtol=1e-5, atol=1e-6)
        _bits(arr.get('actions', n).reshape(n, case.H, case.act), o.sample_actions(ms[0], ms[1], lb, ub, eps[it][:n]),
              'iteration %d reads rows j < n of slab it' % it)
        pl.plan_select(it)
    pl.plan_end()
    pl.close()


def test_with_the_softmax_refit():
    case = dc.BY_NAME['lean']
    pb, pl = _planner(case)
    pl.set_refit('softmax', 0.5)
    arr = Arrays(pl, case)
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(I):
        n = case.schedule[it]
        ms = _np(pl.mu_sigma())
        pl.plan_rollout(it)
        pl.plan_select(it)
        acts, scores = arr.get('actions', n).reshape(n, case.H, case.act), arr.get('scores', n)
        mu, sigma = softmax_refit(scores, _np(pl.elite_idx()), acts, ms[0], ms[1], 0.0, 0.5)[:2]
        got = _np(pl.mu_sigma())
        np.testing.assert_allclose(got[0], mu, rtol=2e-5, atol=2e-6, err_msg='iteration %d' % it)
        np.testing.assert_allclose(got[1], sigma, rtol=2e-4, atol=2e-6, err_msg='iteration %d' % it)
    pl.plan_end()
    pl.close()


def _combined(name):
    lean, safe = dc.BY_NAME['lean'], dc.BY_NAME['two_blocks_safe']
    if name == 'risk_level':
        return lean, lambda pl: pl.set_particle_objective('lower_tail', 2)
    if name == 'cost_budget':
        def budget(pl):
            pl.set_constraint('budget', 0)
            pl.set_cost_budget(0.5)
        return safe, budget
    if name == 'warm_start':
        def warm(pl):
            pl.set_warm_start(shift=1, tail='box', sigma='keep', floor_frac=0.25)
            pl.set_init_mode('shift')
        return lean, warm
    if name == 'everything':
        def every(pl):
            pl.set_elite_carry(3, True, 1)
            pl.set_action_noise('powerlaw', 2.0)
            pl.set_refit('softmax', 0.5)
            pl.set_mean_candidate(True)
        return lean, every
    raise KeyError(name)


@pytest.mark.parametrize('name', ['risk_level', 'cost_budget', 'warm_start', 'everything'])
def test_together_with_the_other_settings_graph_equals_stepwise(name):
    """What this compares is the library with itself: a mistake in the host path the three forms share is held by
    tests/test_gpu_option_fuzz.py, which checks option combinations stage by stage against the composed restatement of tests/composed_cases.py."""
    case, setup = _combined(name)
    pb, ps = _planner(case)
    pb, pg = _planner(case, use_graph=True)
    for pl in (ps, pg):
        setup(pl)
        assert pl.population_schedule() == (list(case.schedule), True)             # the other setters leave it on
        _zero_arrays(pl)
    for j in range(2):
        want = _stepwise(ps, pb['state'], call=CALL + j)
        got = pg.plan(pb['state'], seed=SEED, call=CALL + j)
        _same_plan(got, want, _left(pg), _left(ps), '%s, plan %d' % (name, j))
        assert pg.graph_status() == 'graph'
    ps.close(); pg.close()


# ------------------------------------------------------------------------------------------------- 7: the mean candidate
@pytest.mark.parametrize('name,schedule,iters,m', [('lean', 'case', I, 0), ('ragged', 'case', I, 0), ('lean', None, I, 0), ('lean', None, 1, 0),
                                                   ('lean', 'case', I, 3), ('segments', 'case', I, 0)])
def test_mean_candidate_launch_by_launch(name, schedule, iters, m):
    """Teeth.  Row n - 1 of both layouts is the mirror's in the last iteration only; every other row is the sampler's (or the inject's);
    the other iterations keep their path and launches."""
    case = dc.BY_NAME[name]
    pb, ref = _planner(case, schedule=schedule, I=iters)
    pb, pl = _planner(case, schedule=schedule, mean=True, I=iters)
    if m:
        for p in (ref, pl):
            p.set_elite_carry(m)
    assert pl.mean_candidate() is True
    sched = list(case.schedule) if schedule == 'case' else [case.N] * iters
    lb, ub, _, _ = o.sampling_params(pb['low'], pb['high'])
    pf, psft = dc.pad_layout(case)
    arr, arr_ref = Arrays(pl, case), Arrays(ref, case)
    for it in range(iters):
        a, b = pl.iteration_plan(it), ref.iteration_plan(it)
        if it < iters - 1:
            assert a == b, it
        else:
            # + the kernel, + the sampler launch where the rollout's tiles had sampled (these shapes: all tiles resident, the reduce folded)
            assert b['launches'] == (2 if not m else 5), b
            assert a['rollout_path'] == 'generic' and a['launches'] == b['launches'] + (1 if m else 2), (a, b)
            assert dict(a, launches=0, rollout_path='') == dict(b, launches=0, rollout_path='')
    ea = _np(pl.fill_noise(seed=SEED, call=CALL)[0])
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    ref.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(iters):
        n = sched[it]
        ms = _np(pl.mu_sigma())
        _bits(ms, _np(ref.mu_sigma()), 'iteration %d starts from the same distribution' % it)
        pl.plan_rollout(it); ref.plan_rollout(it)
        acts = arr.get('actions', n).reshape(n, case.H, case.act)
        racts = arr_ref.get('actions', n).reshape(n, case.H, case.act)
        pad = arr.get('act_pad', n).reshape(n, case.H, pf)
        if it < iters - 1:
            _bits(acts, racts, 'iteration %d: no mean candidate' % it)
            _bits(arr.get('scores', n), arr_ref.get('scores', n), 'iteration %d: scores' % it)
        else:
            _bits(acts, mean_candidate(racts, ms[0], lb, ub), 'the last iteration: planner.mean_candidate')
            _bits(acts[:n - 1], racts[:n - 1], 'every other row is what it was')
            if not m:
                _bits(racts, o.sample_actions(ms[0], ms[1], lb, ub, ea[it][:n]), 'the sampler\'s draw')
            assert not np.array_equal(acts[n - 1], racts[n - 1])                  # (the kernel is live)
            np.testing.assert_array_equal(acts[n - 1], np.clip(ms[0], lb, ub))
        if pl.iteration_plan(it)['rollout_path'] == 'generic':                   # (the lean kernels draw in place and keep no padded copy)
            _bits(pad[:, :, psft:psft + case.act], acts, 'iteration %d: the padded quads at the action words' % it)
        rest = np.ones(pf, bool)
        rest[psft:psft + case.act] = False
        assert not pad[:, :, rest].view(U).any(), 'iteration %d: a padding word is not zero' % it
        pl.plan_select(it); ref.plan_select(it)
    r = pl.plan_end()
    ref.plan_end()
    assert r[2] == iters and np.isfinite(r[1])
    pl.close(); ref.close()


@pytest.mark.parametrize('seed', dc.BY_NAME['lean'].oracle_seeds)
def test_mean_candidate_against_the_oracle_replay(seed):
    case = dc.BY_NAME['lean']
    pb, pl = _planner(case, mean=True)
    ra, rs, rit, trace = dc.oracle_plan(case, seed, with_mean=True)
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.P, case.obs, seed=seed)
    arr = Arrays(pl, case)
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    for it in range(I):
        n = case.schedule[it]
        pl.plan_rollout(it)
        np.testing.assert_allclose(arr.get('actions', n).reshape(n, case.H, case.act), trace[it]['actions'], rtol=1e-5, atol=1e-6)
        err = np.abs(arr.get('scores', n) - trace[it]['scores'])
        flipped = err > SCORE_ATOL + 6e-8 * np.abs(trace[it]['scores'])
        assert flipped.mean() <= 0.03 and (not flipped.any() or err[flipped].min() > 1e-3), (it, err.max())
        pl.plan_select(it)
        np.testing.assert_array_equal(np.sort(_np(pl.elite_idx())), np.sort(trace[it]['elite']), err_msg='iteration %d: elite set' % it)
    a, s, n_it = pl.plan_end(eps_out=eo)
    assert n_it == rit == I and abs(s - rs) <= SCORE_ATOL
    np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-7)
    pl.close()


# ------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_leave_the_previous_setting():
    case = dc.BY_NAME['lean']
    pb, pl = _planner(case, schedule=None)
    lib, h = pl.lib, pl.h
    first = [64, 32, 16]

    def st(n, count=None):
        a = (ctypes.c_int32 * len(n))(*n)
        return lib.cem_planner_set_population_schedule(h, a, len(n) if count is None else count)

    def held(sched, on):
        return pl.population_schedule() == (sched, on)
    assert st(first) == 0 and held(first, True)
    plans = [pl.iteration_plan(it) for it in range(I)]
    assert st([64, 32]) == INVALID_ARG and st([64, 32, 16, 8]) == INVALID_ARG and st(first, 2) == INVALID_ARG     # count is 0 or `iterations`
    assert st([64, 32, case.k - 1]) == INVALID_ARG and st([65, 32, 16]) == INVALID_ARG and st([64, 0, 16]) == INVALID_ARG
    assert held(first, True) and [pl.iteration_plan(it) for it in range(I)] == plans
    out = (ctypes.c_int32 * I)()
    assert lib.cem_planner_get_population_schedule(h, out, I - 1, None) == INVALID_ARG
    assert lib.cem_planner_iteration_plan(h, I, ctypes.byref(_capi.CemIterationPlan())) == INVALID_ARG
    assert lib.cem_planner_iteration_plan(h, -1, ctypes.byref(_capi.CemIterationPlan())) == INVALID_ARG
    assert lib.cem_planner_set_mean_candidate(h, 2) == INVALID_ARG and pl.mean_candidate() is False
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    assert st([64, 48, 32]) == STATE and st([]) == STATE and lib.cem_planner_set_mean_candidate(h, 1) == STATE
    assert held(first, True) and pl.mean_candidate() is False
    assert lib.cem_plan_select(h, I) == INVALID_ARG
    pl.plan_rollout(0); pl.plan_select(0); pl.plan_end()
    # carry-over: every population must be wider than n_keep, the mean candidate's row must not be an injected one — either order
    pl.set_elite_carry(8)
    assert st([64, 32, 8]) == UNSUPPORTED and held(first, True)
    assert _status(pl.set_elite_carry, 16) == INVALID_ARG                          # (n_keep > n_elite, as before)
    assert st([64, 32, 9]) == 0
    assert lib.cem_planner_set_mean_candidate(h, 1) == UNSUPPORTED and pl.mean_candidate() is False      # n_keep 8 >= 9 - 1
    assert st([64, 32, 10]) == 0 and lib.cem_planner_set_mean_candidate(h, 1) == 0
    assert st([64, 32, 9]) == UNSUPPORTED and held([64, 32, 10], True)
    pl.set_elite_carry(0)
    assert st([64, 32, 8]) == 0
    assert _status(pl.set_elite_carry, 8) == UNSUPPORTED and _status(pl.set_elite_carry, 7) == UNSUPPORTED and pl.elite_carry()[0] == 0
    assert _status(pl.set_elite_carry, 6) == 0                                    # 6 < 8 - 1
    pl.set_elite_carry(0); pl.set_mean_candidate(False)
    # a communicator on a scheduled handle, and on one with the mean candidate alone
    comm_id = ctypes.create_string_buffer(_capi.CEM_COMM_ID_BYTES)
    assert lib.cem_planner_comm_init(h, comm_id, 1, 0) == UNSUPPORTED
    pl.set_population_schedule(None); pl.set_mean_candidate(True)
    assert lib.cem_planner_comm_init(h, comm_id, 1, 0) == UNSUPPORTED
    pl.close()
    # P n not a multiple of E
    sm = dc.BY_NAME['split_members']
    pbs, psm = _planner(sm, schedule=None)
    assert _status(psm.set_population_schedule, [66, 44, 30]) == INVALID_ARG and _status(psm.set_population_schedule, [66, 45, 30]) == 0
    psm.close()
    # outside the one-workgroup select, sharded, batch handles — and switching OFF is always taken
    for mode in (2, 3):
        pbm, pm = _planner(case, schedule=None, select_mode=mode)
        assert _status(pm.set_population_schedule, first) == UNSUPPORTED and _status(pm.set_mean_candidate, True) == UNSUPPORTED
        assert _status(pm.set_population_schedule, None) == 0 and _status(pm.set_population_schedule, [case.N] * I) == 0
        assert pm.population_schedule() == ([case.N] * I, False) and pm.mean_candidate() is False
        pm.close()
    pbw, pw = _planner(case, schedule=None, world_size=2, rank=0)
    assert _status(pw.set_population_schedule, first) == UNSUPPORTED and _status(pw.set_mean_candidate, True) == UNSUPPORTED
    pw.close()
    _, pcfg = hp.configs(pb, **dc.config_kwargs(case))
    bp = BatchCemPlanner(pcfg, 2)
    assert _status(bp.set_population_schedule, first) == UNSUPPORTED and _status(bp.set_mean_candidate, True) == UNSUPPORTED
    assert bp.population_schedule() == ([case.N] * I, False)
    bp.close()


# ------------------------------------------------------------------------------------------------- 9: policies
def _obs(scale=1.0):
    st = np.zeros(60, F); st[3:19] = 0.5; st[22:38] = 0.6                          # PointGoal1's goal and hazard lidars (tests/test_gpu_warm_start.py)
    return (st * F(scale)).astype(F)


def _policy(cls_name, seed=11, **kw):
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    name = {'CemMpc': 'cem_mpc', 'SafeCemMpc': 'safe_cem_mpc'}[cls_name]
    env, model, _ = make_agent_parts(name, seed=seed)
    trained_like(model, np.random.default_rng(seed))
    cls = {'CemMpc': CemMpc, 'SafeCemMpc': SafeCemMpc}[cls_name]
    return env, model, cls(model=model, environment=env, **dict(POLICIES_YAML[name], iterations=3, **kw))


@pytest.fixture
def planner_cache_as_found():
    """The policies take their handles from the shape-keyed cache (planner.cached_planner).  What these tests add leaves with them, and
    what they pushed out comes back: later tests find the cache as they would have without this file."""
    from ethz_safe_learning_amd import planner
    before = list(planner._PLANNER_CACHE.items())
    yield
    planner._PLANNER_CACHE.clear()
    planner._PLANNER_CACHE.update(before)


@pytest.mark.parametrize('cls_name', ['CemMpc', 'SafeCemMpc'])
def test_policies_plan_with_population_decay_and_the_mean_candidate(cls_name, planner_cache_as_found):
    _torch()
    env, model, pol = _policy(cls_name, population_decay=1.25, mean_candidate=True)
    env, model, plain = _policy(cls_name)
    sched = population_schedule(pol.n_samples, pol.elite, 3, 1.25, pol.particles, model.model.ensemble_size)
    assert sched[0] == pol.n_samples and sched[-1] < pol.n_samples
    obs = _obs()
    a = pol.generate_action(obs)
    assert a.shape == (2,) and np.isfinite(a).all() and np.isfinite(pol.last_score)
    assert pol._planner.population_schedule() == (sched, True) and pol._planner.mean_candidate() is True
    assert pol.planner_config().population == tuple(sched) and pol.planner_config().mean_candidate is True
    plain.generate_action(obs)
    assert plain._planner is not pol._planner and plain._planner.population_schedule()[1] is False     # another configuration, another handle
    assert plain.planner_config().population == () and plain.planner_config().mean_candidate is False
    with pytest.raises(ValueError, match='batch'):
        pol.generate_actions(np.stack([obs, _obs(0.9)]))
    if cls_name == 'SafeCemMpc':
        pol.optimize_for_safety(obs)
        assert pol._cost_planner.population_schedule() == (sched, True) and pol._cost_planner.mean_candidate() is True
    with pytest.raises(ValueError):
        _policy(cls_name, population_decay=0.9)
    with pytest.raises(ValueError):
        _policy(cls_name, min_population=10)                                      # needs population_decay
