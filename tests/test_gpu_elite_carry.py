"""Elite carry-over (cem_planner_set_elite_carry) on the device.

The two kernels have exact references that cost nothing: planner.keep_elites and planner.inject_elites are comparisons and copies, the
sampler's draw is oracle.sample_actions on the handle's own mu / sigma and the dumped Philox stream (bit for bit, as
tests/test_gpu_bounds.py holds it), and the store is readable after every launch (elite_store).  So the stepwise form is checked launch by
launch over tests/elite_cases.py (1, 2), and everything else — early stop, the three plan forms, batch handles, across plans, off is
off, the oracle, the other settings, refusals, policies — hangs off that."""
import ctypes

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd import BatchCemPlanner, _capi
from ethz_safe_learning_amd.planner import elite_keep_count, inject_elites, keep_elites
from tests import elite_cases as ec
from tests import helpers as hp
from tests import select_cases as sc

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
SCORE_ATOL = 2e-5                        # tests/test_gpu_parity.py FULL_SIZE_ATOL, tests/test_gpu_whole_plan.py SCORE_ATOL
SEED, CALL = ec.PLAN_SEED, ec.PLAN_CALL
I = ec.I
IDS = [c.name for c in ec.CASES]


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


def _planner(case, m=None, across=False, shift=None, **over):
    """A handle of the case (m = 0: carry-over never enabled)."""
    _torch()
    pb = ec.problem(case)
    _, pcfg = hp.configs(pb, **ec.config_kwargs(case, **over))
    pl = hp.make_planner(pb, pcfg)
    m = case.m if m is None else m
    if m:
        pl.set_elite_carry(m, across, case.shift if shift is None else shift)
    return pb, pl


def _pad(pl, case):
    """act_pad of problem 0 as floats [N, H, pad_floats]."""
    pf, _ = ec.pad_layout(case)
    off = ec.pad_offset(pl.layout.actions, case, pl.max_batch)
    pl.synchronize()
    return _np(pl._ws_view[off:off + case.N * case.H * pf * 4].view(_torch().float32)).reshape(case.N, case.H, pf)


def _check_pad(pl, case, acts, what):
    pf, ps = ec.pad_layout(case)
    pad = _pad(pl, case)
    _bits(pad[:, :, ps:ps + case.act], acts, '%s: the padded quads at the action words' % what)
    rest = np.ones(pf, bool)
    rest[ps:ps + case.act] = False
    assert not pad[:, :, rest].view(U).any(), '%s: a padding word is not zero' % what


def _left(pl):
    E, count = pl.elite_store()
    return dict(mu_sigma=_np(pl.mu_sigma()), elite_idx=_np(pl.elite_idx()), actions=_np(pl.actions()), store=E, count=np.int32(count))


def _same_plan(got, want, left_got, left_want, what):
    _bits(got[0], want[0], '%s: action' % what)
    assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2], (what, got, want)
    for key in left_want:
        _bits(left_got[key], left_want[key], '%s: %s' % (what, key))


def _stepwise(pl, state, seed=SEED, call=CALL, iters=I, **noise):
    pl.plan_begin(state, seed=seed, call=call, **noise)
    for it in range(iters):
        pl.plan_rollout(it)
        pl.plan_select(it)
    return pl.plan_end()


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except _capi.CemError as e:
        return e.status
    return 0


# ------------------------------------------------------------------------------------------------- 1, 2: the two kernels, launch by launch
@pytest.mark.parametrize('case', ec.CASES, ids=IDS)
def test_inject_and_keep_launch_by_launch(case):
    """Teeth.  After every rollout call: rows < m are the store the previous select left, rows >= m the sampler's draw, both layouts alike;
    after every select call: the store is keep_elites of what the select ranked."""
    pb, pl = _planner(case)
    m, H, A = case.m, case.H, case.act
    assert pl.elite_carry() == (m, False, case.shift) and pl.rollout_path() == 'generic'
    lb, ub, _, _ = o.sampling_params(pb['low'], pb['high'])
    ea = _np(pl.fill_noise(seed=SEED, call=CALL)[0])
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    assert pl.elite_store()[1] == 0                                               # nothing kept yet (readable inside a stepwise plan)
    store = None
    for it in range(I):
        ms = _np(pl.mu_sigma())
        pl.plan_rollout(it)
        acts = _np(pl.actions())
        drawn = o.sample_actions(ms[0], ms[1], lb, ub, ea[it])
        if it == 0:
            _bits(acts, drawn, 'iteration 0: the plain sampler')
        else:
            _bits(acts[:m], store, 'iteration %d: rows < m are the store' % it)
            _bits(acts[m:], drawn[m:], 'iteration %d: rows >= m are the draw' % it)
            _bits(acts, inject_elites(drawn, store, m, 0), 'iteration %d: inject_elites' % it)
            assert not np.array_equal(acts[:m], drawn[:m])                        # (the inject is live)
        _check_pad(pl, case, acts, 'iteration %d' % it)
        pl.plan_select(it)
        store, count = pl.elite_store()
        assert count == m and store.shape == (m, H, A)
        scores, elite = _np(pl.scores_global()), _np(pl.elite_idx())
        _bits(store, keep_elites(scores, elite, acts, m), 'iteration %d: keep_elites' % it)
        _bits(_np(pl.actions()), acts, 'iteration %d: the keep only reads the sample' % it)
    a, s, n_it = pl.plan_end()
    assert n_it == I and np.isfinite(s)
    pl.close()


ADVERSARIAL = [(c, c.m) for c in ec.CASES] + [(ec.BY_NAME['lean_one_quad'], m) for m in (1, ec.K)]       # every case at its own m, and m = 1, k


@pytest.mark.parametrize('case,m', ADVERSARIAL, ids=['%s_m%d' % (c.name, m) for c, m in ADVERSARIAL])
def test_keep_on_adversarial_scores(case, m):
    """Teeth.  The launch-by-launch run again with scores_local overwritten between rollout and select, in iteration 0 and in iteration 1
    (whose sample holds injected rows): ties across the m-th place, both zeros, NaN, the infinities.  Every case: both action-quad
    layouts, the select instantiations of all three variants, the wide and split-product handles, floating segments."""
    torch = _torch()
    pb, pl = _planner(case, m=m)
    for name, vec in ec.adversarial_scores(case.N, case.k, m).items():
        pl.plan_begin(pb['state'], seed=SEED, call=CALL)
        for it in range(2):
            pl.plan_rollout(it)
            pl.synchronize()
            with pl.stream_context():
                pl.scores_local(sync=False).copy_(torch.from_numpy(vec))
            acts = _np(pl.actions())
            pl.plan_select(it)
            store, count = pl.elite_store()
            elite = _np(pl.elite_idx())
            np.testing.assert_array_equal(np.sort(elite), sc.reference_top_k(vec, case.k), err_msg='%s iteration %d' % (name, it))
            assert count == m
            _bits(store, keep_elites(vec, elite, acts, m), '%s iteration %d' % (name, it))
        pl.plan_end()
    pl.close()


# ------------------------------------------------------------------------------------------------- 3: early stop
def test_early_stop_leaves_the_store_of_the_last_iteration_that_ran():
    case = ec.BY_NAME['lean_one_quad']
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
    pb, pl = _planner(case, thr=thr)
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(2):
        pl.plan_rollout(it)
        pl.plan_select(it)
    want = _left(pl)                                                              # the select that set `done` has kept
    assert want['count'] == case.m
    _bits(want['store'], keep_elites(_np(pl.scores_global()), want['elite_idx'], want['actions'], case.m))
    pl.plan_rollout(2)                                                            # sampler, inject, rollout, select, keep: all leave at once
    pl.plan_select(2)
    got = _left(pl)
    for key in want:
        _bits(got[key], want[key], 'after the iteration that did not run: %s' % key)
    a, s, n_it = pl.plan_end()
    assert n_it == 2
    pb, pe = _planner(case, thr=thr)
    r = pe.plan(pb['state'], seed=SEED, call=CALL)
    _same_plan(r, (a, s, n_it), _left(pe), want, 'the eager plan that stops early')
    pl.close(); pe.close()


# ------------------------------------------------------------------------------------------------- 4: the plan forms agree
@pytest.mark.parametrize('case', ec.CASES, ids=IDS)
def test_graph_eager_and_stepwise_plans_agree(case):
    pb, ps = _planner(case)
    want = _stepwise(ps, pb['state'])
    left = _left(ps)
    pb, pe = _planner(case)
    _same_plan(pe.plan(pb['state'], seed=SEED, call=CALL), want, _left(pe), left, 'eager')
    assert pe.graph_status() == 'eager'
    pb, pg = _planner(case, use_graph=True)
    for rep in range(2):                                                          # captured, then replayed: a replay starts from what the last plan left
        _same_plan(pg.plan(pb['state'], seed=SEED, call=CALL), want, _left(pg), left, 'graph, plan %d' % rep)
        assert pg.graph_status() == 'graph'
    for p in (ps, pe, pg):
        p.close()


@pytest.mark.parametrize('name,use_graph', [('lean_one_quad', True), ('safe', False), ('two_quads', True)])
def test_batch_problems_equal_their_single_plans(name, use_graph):
    torch = _torch()
    case = ec.BY_NAME[name]
    pb = ec.problem(case)
    _, pcfg = hp.configs(pb, **ec.config_kwargs(case, use_graph=use_graph))
    cap, n = 4, 3                                                                 # n_states < max_batch
    rng = np.random.default_rng(3)
    states = (pb['state'][None] + rng.normal(0, 0.05, (n, case.obs))).astype(F)
    calls = np.array([CALL, CALL + 7, (2 << 32) + 1], np.uint64)
    bp = BatchCemPlanner(pcfg, cap)
    bp.set_weights(pb['weights']); bp.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    bp.set_elite_carry(case.m)
    assert _status(bp.set_elite_carry, case.m, True, 1) == UNSUPPORTED            # across plans: not on a batch handle
    assert bp.elite_carry() == (case.m, False, 1)                                 # the refused call left the setting
    for rep in range(2):
        acts, scores, iters = bp.plan_batch(states, seed=SEED, calls=calls)
    singles = []
    for b in range(n):
        _, pl = _planner(case)
        r = pl.plan(states[b], seed=SEED, call=int(calls[b]))
        E, count = pl.elite_store()
        singles.append((r, E, count))
        pl.close()
    for b in range(n):
        (a, s, it), E, count = singles[b]
        _bits(acts[b], a, 'problem %d: action' % b)
        assert F(scores[b]).view(U) == F(s).view(U) and iters[b] == it
        Eb, cb = bp.elite_store(b)
        assert cb == count == case.m
        _bits(Eb, E, 'problem %d: store' % b)
    Et, ct = bp.elite_store(cap - 1)                                              # the slot that sat both plans out keeps its bytes
    assert ct == 0 and not Et.view(U).any()
    assert _status(bp.elite_store, cap) == INVALID_ARG
    torch.cuda.synchronize()
    bp.close()


# ------------------------------------------------------------------------------------------------- 5: across plans
@pytest.mark.parametrize('case', ec.ACROSS_CASES, ids=[c.name for c in ec.ACROSS_CASES])
def test_across_plans_the_first_iteration_takes_the_shifted_store(case):
    pb, pl = _planner(case, across=True)
    m, H, s = case.m, case.H, case.shift
    assert pl.elite_carry() == (m, True, s)
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    mu0, sg0 = np.broadcast_to(mu0, (H, case.act)), np.broadcast_to(sg0, (H, case.act))

    def first_iteration(call):
        """(iteration-0 sample of a stepwise plan with this call number, the sampler's draw); the plan is run to its end."""
        ea = _np(pl.fill_noise(seed=SEED, call=call)[0])
        pl.plan_begin(pb['state'], seed=SEED, call=call)
        pl.plan_rollout(0)
        acts = _np(pl.actions())
        _check_pad(pl, case, acts, 'call %d iteration 0' % call)
        pl.plan_select(0)
        for it in range(1, I):
            pl.plan_rollout(it)
            pl.plan_select(it)
        pl.plan_end()
        return acts, o.sample_actions(mu0, sg0, lb, ub, ea[0])

    acts, drawn = first_iteration(CALL)
    _bits(acts, drawn, 'the first plan: nothing to take')
    final, count = pl.elite_store()
    assert count == m
    acts, drawn = first_iteration(CALL + 1)
    _bits(acts[:m, :H - s], final[:, s:], 'the second plan: the store moved %d steps' % s)
    _bits(acts[:m, H - s:], drawn[:m, H - s:], 'the second plan: the freed tail is the draw')
    _bits(acts[m:], drawn[m:], 'the second plan: rows >= m')
    _bits(acts, inject_elites(drawn, final, m, s), 'inject_elites')
    # the three ways the count goes back to zero
    pl.reset_carry()
    assert pl.elite_store()[1] == 0
    acts, drawn = first_iteration(CALL + 2)
    _bits(acts, drawn, 'after reset_carry')
    pl.set_elite_carry(m, True, s)
    assert pl.elite_store()[1] == 0
    acts, drawn = first_iteration(CALL + 3)
    _bits(acts, drawn, 'after a setter call')
    assert pl.elite_store()[1] == m
    pl.set_init_mode('explicit')                                                  # a plan call that fails: EXPLICIT without an upload
    assert _status(pl.plan, pb['state'], seed=SEED, call=CALL + 4) == STATE
    pl.set_init_mode('cold')
    acts, drawn = first_iteration(CALL + 5)
    _bits(acts, drawn, 'after a failed plan')
    # set_weights / set_normaliser keep the store
    final, _ = pl.elite_store()
    pl.set_weights(pb['weights']); pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    acts, drawn = first_iteration(CALL + 6)
    _bits(acts, inject_elites(drawn, final, m, s), 'after set_weights and set_normaliser')
    pl.close()


def test_across_plans_one_graph_serves_the_first_and_later_plans():
    case = ec.BY_NAME['lean_one_quad']
    pb, ps = _planner(case, across=True)
    pb, pg = _planner(case, across=True, use_graph=True)
    pb, pe = _planner(case, across=True)
    rng = np.random.default_rng(4)
    for j in range(3):
        st = (pb['state'] + rng.normal(0, 0.05, case.obs)).astype(F)
        want = _stepwise(ps, st, call=CALL + j)
        left = _left(ps)
        _same_plan(pg.plan(st, seed=SEED, call=CALL + j), want, _left(pg), left, 'graph, plan %d' % j)
        _same_plan(pe.plan(st, seed=SEED, call=CALL + j), want, _left(pe), left, 'eager, plan %d' % j)
        assert pg.graph_status() == 'graph'
    for p in (ps, pg, pe):
        p.close()


# ------------------------------------------------------------------------------------------------- 6: off is off
def test_off_is_off_and_the_lean_path_comes_back():
    case = ec.BY_NAME['lean_one_quad']
    pb, fresh = _planner(case, m=0, use_graph=True)
    pb, pl = _planner(case, m=0, use_graph=True)
    assert fresh.rollout_path() == pl.rollout_path() == 'lean' and case.lean
    base = fresh.launches_per_iteration()
    assert base == 2                                                              # the rollout (which samples) and the select (which reduces)
    assert pl.elite_carry() == (0, False, 1) and _status(pl.elite_store) == STATE
    pl.set_elite_carry(case.m)
    assert pl.rollout_path() == 'generic' and pl.launches_per_iteration() == base + 3      # + the sampler launch, the inject, the keep
    pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.elite_store()[1] == case.m
    pl.set_elite_carry(0)
    assert pl.rollout_path() == 'lean' and pl.launches_per_iteration() == base and pl.elite_carry()[0] == 0
    want = fresh.plan(pb['state'], seed=SEED, call=CALL)
    got = pl.plan(pb['state'], seed=SEED, call=CALL)
    _bits(got[0], want[0], 'action')
    assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2]
    for key in ('mu_sigma', 'elite_idx', 'actions'):
        _bits(_np(getattr(pl, key)()), _np(getattr(fresh, key)()), key)
    assert pl.graph_status() == 'graph'
    # a handle that keeps its reduce kernel: the same three launches more
    case2 = ec.BY_NAME['safe']
    pb2, p2 = _planner(case2, m=0)
    n0, path0 = p2.launches_per_iteration(), p2.rollout_path()
    p2.set_elite_carry(case2.m)
    assert p2.launches_per_iteration() == n0 + 3 and p2.rollout_path() == 'generic'
    p2.set_elite_carry(0)
    assert (p2.launches_per_iteration(), p2.rollout_path()) == (n0, path0)
    for p in (fresh, pl, p2):
        p.close()


# ------------------------------------------------------------------------------------------------- 7: the oracle
@pytest.mark.parametrize('case,seed', ec.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in ec.ORACLE_CASES])
def test_whole_plan_against_the_oracle(case, seed):
    """sample -> inject -> scores -> select and refit -> keep replayed by the fp32 oracle on the same noise tensors.  The seeds keep both
    cuts wider than ec.ORACLE_GAP in the oracle (tests/test_elite_cases_cpu.py), so the elite sets and the kept rows must be EQUAL."""
    pb, pl = _planner(case)
    ra, rs, rit, trace = ec.oracle_plan(case, seed)
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.E, case.obs, seed=seed)
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    for it in range(I):
        pl.plan_rollout(it)
        acts, scores = _np(pl.actions()), _np(pl.scores_local())
        np.testing.assert_allclose(acts, trace[it]['actions'], rtol=1e-5, atol=1e-6, err_msg='iteration %d: actions' % it)
        err = np.abs(scores - trace[it]['scores'])
        print('%s seed %d iteration %d: max score error %.3g' % (case.name, seed, it, err.max()))
        # (a `<=` of the objective may resolve differently within rounding and move a score by a whole unit: rare, and never on a cut)
        flipped = err > SCORE_ATOL + 6e-8 * np.abs(trace[it]['scores'])
        assert flipped.mean() <= 0.03 and (not flipped.any() or err[flipped].min() > 1e-3), 'iteration %d: %d scores off, by %.3g at least' % (
            it, flipped.sum(), err[flipped].min() if flipped.any() else 0.0)
        pl.plan_select(it)
        elite = _np(pl.elite_idx())
        np.testing.assert_array_equal(np.sort(elite), np.sort(trace[it]['elite']), err_msg='iteration %d: elite set' % it)
        store, count = pl.elite_store()
        assert count == case.m
        _bits(store, keep_elites(trace[it]['scores'], trace[it]['elite'], acts, case.m), 'iteration %d: the oracle keeps the same rows' % it)
        np.testing.assert_allclose(store, trace[it]['store'], rtol=1e-5, atol=1e-6)
        ms = _np(pl.mu_sigma())
        np.testing.assert_allclose(ms[0], trace[it]['mu'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(ms[1], trace[it]['sigma'], rtol=1e-5, atol=1e-6)
    a, s, n_it = pl.plan_end(eps_out=eo)
    assert n_it == rit == I
    np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-7)
    assert abs(s - rs) <= SCORE_ATOL
    # the same tensors through the whole-plan call
    r = pl.plan(pb['state'], eps_act=ea, eps_model=em, eps_out=eo)
    _bits(r[0], a, 'the eager tensor-fed plan'); assert F(r[1]).view(U) == F(s).view(U)
    pl.close()


# ------------------------------------------------------------------------------------------------- 8: together with the other settings
def _combined(name):
    safe = ec.BY_NAME['safe']
    lean = ec.BY_NAME['lean_one_quad']
    if name == 'elite_temperature':
        return lean, lambda pl: pl.set_refit('softmax', 0.5)
    if name == 'noise_beta':
        return lean, lambda pl: pl.set_action_noise('powerlaw', 1.0)
    if name == 'warm_start':
        def warm(pl):
            pl.set_warm_start(shift=1, tail='box', sigma='keep', floor_frac=0.25)
            pl.set_init_mode('shift')
        return lean, warm
    if name == 'risk_level':
        return lean, lambda pl: pl.set_particle_objective('lower_tail', 2)
    if name == 'cost_budget':
        def budget(pl):
            pl.set_constraint('budget', 0)
            pl.set_cost_budget(0.5)
        return safe, budget
    raise KeyError(name)


@pytest.mark.parametrize('name', ['elite_temperature', 'noise_beta', 'warm_start', 'risk_level', 'cost_budget'])
def test_together_with_the_other_settings_graph_equals_stepwise(name):
    """What this compares is the library with itself: a mistake in the host path the three forms share is held by
    tests/test_gpu_option_fuzz.py, which checks option combinations stage by stage against the composed restatement of tests/composed_cases.py."""
    case, setup = _combined(name)
    across = name == 'warm_start'                                                 # a warm-started policy shifts its elites too
    pb, ps = _planner(case, across=across)
    pb, pg = _planner(case, across=across, use_graph=True)
    for pl in (ps, pg):
        setup(pl)
        assert pl.elite_carry()[0] == case.m                                      # the other setters leave it on
    for j in range(2):
        want = _stepwise(ps, pb['state'], call=CALL + j)
        got = pg.plan(pb['state'], seed=SEED, call=CALL + j)
        _same_plan(got, want, _left(pg), _left(ps), '%s, plan %d' % (name, j))
        assert pg.graph_status() == 'graph'
    ps.close(); pg.close()


# ------------------------------------------------------------------------------------------------- 9: refusals
def test_refusals():
    case = ec.BY_NAME['lean_one_quad']
    pb, pl = _planner(case, m=0)
    lib, h = pl.lib, pl.h

    def st(n_keep, across=0, shift=1, reserved=0):
        c = _capi.CemEliteCarry(n_keep=n_keep, across_plans=across, shift=shift, reserved=reserved)
        return lib.cem_planner_set_elite_carry(h, c)
    assert lib.cem_planner_set_elite_carry(h, None) == INVALID_ARG
    assert st(-1) == INVALID_ARG and st(case.k + 1) == INVALID_ARG
    assert st(1, across=2) == INVALID_ARG and st(1, across=-1) == INVALID_ARG and st(1, reserved=1) == INVALID_ARG
    assert st(1, across=1, shift=0) == INVALID_ARG and st(1, across=1, shift=case.H) == INVALID_ARG
    assert st(1, across=0, shift=0) == 0 and st(1, across=1, shift=case.H - 1) == 0   # shift is read with across_plans only
    assert pl.elite_carry() == (1, True, case.H - 1)
    assert st(case.k + 1) == INVALID_ARG and pl.elite_carry() == (1, True, case.H - 1)      # a refused call leaves the setting
    assert lib.cem_planner_get_elite_carry(h, None) == INVALID_ARG
    assert lib.cem_planner_elite_store(h, 0, None, None) == INVALID_ARG and _status(pl.elite_store, 1) == INVALID_ARG and _status(pl.elite_store, -1) == INVALID_ARG
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    assert st(2) == STATE and pl.elite_carry()[0] == 1
    pl.plan_rollout(0); pl.plan_select(0); pl.plan_end()
    assert st(case.k) == 0 and st(0) == 0
    pl.close()
    # n_keep >= n_samples (k = N is a legal handle: MPPI)
    pb, pk = _planner(case, m=0, k=case.N)
    assert _status(pk.set_elite_carry, case.N) == INVALID_ARG and _status(pk.set_elite_carry, case.N - 1) == 0
    pk.close()
    # more than 4096 elites (the keep's LDS): the one-workgroup select still serves k = 4100 of N = 4200, the keep does not
    pbb, pb4 = _planner(ec.BY_NAME['h1'], m=0, N=4200, k=ec.ELITE_MAX_K + 4)
    assert pb4.select_mode() == 1
    assert _status(pb4.set_elite_carry, 1) == UNSUPPORTED and _status(pb4.set_elite_carry, 0) == 0 and pb4.elite_carry()[0] == 0
    pb4.close()
    pbb, pb4 = _planner(ec.BY_NAME['h1'], m=0, N=4200, k=ec.ELITE_MAX_K)
    assert _status(pb4.set_elite_carry, 1) == 0                                   # ... and k = 4096 is served
    pb4.close()
    # H = 1: no shift fits
    h1 = ec.BY_NAME['h1']
    pb1, p1 = _planner(h1)
    assert _status(p1.set_elite_carry, h1.m, True, 1) == INVALID_ARG and p1.elite_carry() == (h1.m, False, 1)
    p1.close()
    # outside the one-workgroup select, sharded, and a communicator on an enabled handle
    for mode in (2, 3):
        pbm, pm = _planner(case, m=0, select_mode=mode)
        assert _status(pm.set_elite_carry, 1) == UNSUPPORTED and _status(pm.set_elite_carry, 0) == 0
        pm.close()
    pbw, pw = _planner(case, m=0, world_size=2, rank=0)
    assert _status(pw.set_elite_carry, 1) == UNSUPPORTED
    pw.close()
    pbc, pc = _planner(case)
    comm_id = ctypes.create_string_buffer(_capi.CEM_COMM_ID_BYTES)
    assert pc.lib.cem_planner_comm_init(pc.h, comm_id, 1, 0) == UNSUPPORTED
    pc.close()


# ------------------------------------------------------------------------------------------------- 10: policies
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
    """The policies take their handles from the shape-keyed cache (planner.cached_planner: 32 entries, least recently used out first).
    What these tests add leaves with them, and what they pushed out comes back: later tests find the cache as they would have without
    this file."""
    from ethz_safe_learning_amd import planner
    before = list(planner._PLANNER_CACHE.items())
    yield
    planner._PLANNER_CACHE.clear()
    planner._PLANNER_CACHE.update(before)


@pytest.mark.parametrize('cls_name', ['CemMpc', 'SafeCemMpc'])
def test_policies_keep_elites(cls_name, planner_cache_as_found):
    _torch()
    env, model, pol = _policy(cls_name, keep_elites=0.3)
    env, model, plain = _policy(cls_name)
    m = elite_keep_count(0.3, pol.elite)
    obs = _obs()
    a = pol.generate_action(obs)
    assert a.shape == (2,) and np.isfinite(a).all() and np.isfinite(pol.last_score)
    assert pol._planner.elite_carry() == (m, False, 1) and pol._planner.elite_store()[1] == m
    plain.generate_action(obs)
    assert plain._planner is not pol._planner and plain._planner.elite_carry()[0] == 0      # another configuration, another handle
    assert plain.planner_config().keep_elites == 0 and pol.planner_config().keep_elites == m
    acts = pol.generate_actions(np.stack([obs, _obs(0.9)]))                       # keep_elites alone serves batched plans
    assert acts.shape == (2, 2) and np.isfinite(acts).all()
    if cls_name == 'SafeCemMpc':
        pol.optimize_for_safety(obs)
        assert pol._cost_planner.elite_carry() == (m, False, 1)
    with pytest.raises(ValueError):
        _policy(cls_name, shift_elites=True)                                       # needs keep_elites


def test_policy_shift_elites_through_generate_action_and_reset(planner_cache_as_found):
    _torch()
    env, model, pol = _policy('CemMpc', keep_elites=0.3, shift_elites=True, warm_shift=2)
    env, model, twin = _policy('CemMpc', keep_elites=0.3, shift_elites=True, warm_shift=2)
    m = elite_keep_count(0.3, pol.elite)
    obs = _obs()
    pol.generate_action(obs)
    twin.generate_action(obs)
    assert pol._planner is not twin._planner                                       # the store lives on the handle: one per policy
    assert pol._planner.elite_carry() == (m, True, 2)
    final, count = pol._planner.elite_store()
    assert count == m
    # the next decision starts from those rows, moved two steps: read back through a stepwise plan on the policy's own handle
    pl = pol._planner
    pl.plan_begin(np.asarray(obs, F), seed=pol.seed, call=77)
    pl.plan_rollout(0)
    acts = _np(pl.actions())
    _bits(acts[:m, :pol.horizon - 2], final[:, 2:], 'the policy\'s second plan takes the shifted store')
    pl.plan_select(0); pl.plan_rollout(1); pl.plan_select(1); pl.plan_rollout(2); pl.plan_select(2); pl.plan_end()
    assert pl.elite_store()[1] == m
    pol.reset()
    assert pl.elite_store()[1] == 0 and twin._planner.elite_store()[1] == m        # reset() empties this policy's store alone
    a = pol.generate_action(obs)
    assert np.isfinite(a).all()
    with pytest.raises(ValueError, match='shift_elites'):
        pol.generate_actions(np.stack([obs, obs]))
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    env, model, safe = _policy('SafeCemMpc', keep_elites=0.3, shift_elites=True)
    safe.optimize_for_safety(_obs())
    assert safe._cost_planner.elite_carry() == (elite_keep_count(0.3, safe.elite), False, 1)   # cost plans: within the plan only
    assert isinstance(safe, SafeCemMpc) and safe.planner_config().shift_elites


def test_safe_policies_with_shift_elites_plan_on_handles_of_their_own(planner_cache_as_found):
    """Two SafeCemMpc policies of one shape, neither warm-started nor budgeted: the store lives on the handle, so each has its own, and
    reset() of one leaves the other's elites alone."""
    _torch()
    env, model, pol = _policy('SafeCemMpc', keep_elites=0.3, shift_elites=True)
    env, model, twin = _policy('SafeCemMpc', keep_elites=0.3, shift_elites=True)
    assert not pol.warm_start and pol.cost_budget is None and pol._owns_handles() and twin._owns_handles()
    m = elite_keep_count(0.3, pol.elite)
    obs = _obs()
    pol.generate_action(obs)
    twin.generate_action(_obs(0.9))
    assert pol._planner is not twin._planner
    assert pol._planner.elite_carry() == twin._planner.elite_carry() == (m, True, 1)
    mine, count = pol._planner.elite_store()
    theirs, tcount = twin._planner.elite_store()
    assert count == tcount == m and not np.array_equal(mine, theirs)              # (other observations, other elites)
    # the policy's next plan starts from ITS store: read back through a stepwise plan on its own handle
    pl = pol._planner
    pl.plan_begin(obs, seed=pol.seed, call=77)
    pl.plan_rollout(0)
    _bits(_np(pl.actions())[:m, :pol.horizon - 1], mine[:, 1:], 'the second plan takes the policy\'s own shifted store')
    pl.plan_select(0); pl.plan_rollout(1); pl.plan_select(1); pl.plan_rollout(2); pl.plan_select(2); pl.plan_end()
    pol.reset()
    assert pl.elite_store()[1] == 0 and twin._planner.elite_store()[1] == m
    _bits(twin._planner.elite_store()[0], theirs, 'reset() of one policy leaves the other\'s store')
    # a policy that carries inside plans only shares the shape's handle as before
    env, model, a = _policy('SafeCemMpc', keep_elites=0.3)
    env, model, b = _policy('SafeCemMpc', keep_elites=0.3)
    a.generate_action(obs); b.generate_action(obs)
    assert a._planner is b._planner and not a._owns_handles()
