"""The lower-tail particle objective on the device (cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL; csrc/cem_score.h)
against its NumPy restatement (tests/risk_cases.py).

Every expected score is computed from the handle's OWN returns() and costs() of the same rollout: a stable sort, a sequential fp32 sum,
one division and cem_reduce_kernel's Beta filter have one right answer, so every comparison is assert_array_equal and no tolerance
exists to be measured."""
import dataclasses

import numpy as np
import pytest

from tests import helpers as hp
from tests import risk_cases as rc

pytestmark = pytest.mark.gpu

O, A = rc.O, rc.A
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7        # enum cem_status: CEM_ERR_INVALID_ARG, CEM_ERR_UNSUPPORTED, CEM_ERR_STATE


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _want(pl, m, safe, thr):
    """The restatement on what the handle's last rollout left: (scores, unsafe flags or None)."""
    ret = _np(pl.returns())
    if not safe:
        return rc.scores(ret, m), None
    costs = _np(pl.costs())
    return rc.scores(ret, m, costs, thr), rc.unsafe_flags(costs, ret.shape[0], thr)


def _planner(pb, variant, thr, worst=0, **kw):
    _, pcfg = rc.configs(pb, worst=worst, variant=variant, post=thr, **kw)
    return hp.make_planner(pb, pcfg)


# ------------------------------------------------------------------------------------------------- 1: stepwise scores and elites
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('case', list(rc.SHAPES))
def test_stepwise_scores_and_elites_equal_the_restatement(case, variant):
    _torch()
    P, N, H, E, thr = rc.SHAPES[case]
    safe, k, I = variant == 'safe', 9, 2
    pb = rc.problem(E=E)
    pl = _planner(pb, variant, thr, N=N, H=H, P=P, E=E, k=k, I=I)
    assert pl.particle_objective() == ('mean', 0)
    ea, em, _ = hp.noise(I, N, H, A, P, O, seed=rc.NOISE_SEED)
    seen_safe = seen_unsafe = False
    for m in rc.tail_ms(P):
        pl.set_particle_objective('lower_tail', m)
        assert pl.particle_objective() == ('lower_tail', m)
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        for it in range(I):
            pl.plan_rollout(it)
            got = _np(pl.scores_local())
            want, unsafe = _want(pl, m, safe, thr)
            np.testing.assert_array_equal(got, want, err_msg='m = %d, iteration %d' % (m, it))
            if safe:
                seen_safe, seen_unsafe = seen_safe or bool((~unsafe).any()), seen_unsafe or bool(unsafe.any())
            pl.plan_select(it)
            np.testing.assert_array_equal(np.sort(_np(pl.elite_idx())), rc.top_k(got, k), err_msg='m = %d, iteration %d' % (m, it))
        pl.plan_end(eps_out=np.zeros(A, np.float32))
        if P > 1 and m == 1:                                           # the worst particle is not the mean
            ret = _np(pl.returns())
            assert (got - (-100 * unsafe if safe else 0) < ret.sum(axis=0, dtype=np.float32) / np.float32(P)).any()
    if safe:
        assert seen_safe and seen_unsafe, 'the threshold of this case should split the candidates'
    pl.close()


# ------------------------------------------------------------------------------------------------- 2: ties
def test_identical_particles_tie_and_every_m_gives_that_return():
    """sampling_propagation off and one member: a candidate's particles are the same rollout, so every m gives return * m / m."""
    _torch()
    P, N, H, E = 5, 70, 8, 1
    pb = rc.problem(E=E)
    pl = _planner(pb, 'cem', 0.5, N=N, H=H, P=P, E=E, k=7, I=1, sampling=False)
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=3)
    for m in rc.tail_ms(P):
        pl.set_particle_objective('lower_tail', m)
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        pl.plan_rollout(0)
        ret, got = _np(pl.returns()), _np(pl.scores_local())
        assert (ret == ret[0]).all() and np.unique(ret[0]).size > 10
        np.testing.assert_array_equal(got, rc.scores(ret, m))
        pl.plan_select(0)
        pl.plan_end(eps_out=np.zeros(A, np.float32))
    pl.close()


def test_planted_equal_returns_through_compute_objective():
    """Trajectory rows copied between particles have equal returns; a handle of ONE particle scores every row by itself
    ((0 + r) / 1 = r), which gives the per-particle returns the restatement needs."""
    torch = _torch()
    P, n, H, E = 5, 70, 6, 5
    pb = rc.problem(E=E)
    rng = np.random.default_rng(2)
    traj = rng.uniform(0.05, 0.95, (P, n, H + 1, O)).astype(np.float32)
    traj[1] = traj[0]                                                  # particles 0 and 1 tie everywhere
    traj[4, ::2] = traj[2, ::2]                                        # 2 and 4 on the even candidates
    traj[3, :10] = traj[0, :10]                                        # three-way on the first ten
    traj = traj.reshape(P * n, H + 1, O)
    NEVER = 0.999                                                      # above the posterior mean of P costs out of P: nothing is unsafe
    for variant, thr in (('cem', 0.5), ('safe', rc._thr(P, 1))):
        # the per-particle returns of this objective (the safe one masks by done first): a one-particle handle that deems nothing unsafe
        one = _planner(pb, variant, NEVER, N=E, H=1, P=1, E=E, k=1, I=1)
        ret = _np(one.compute_objective(traj)).reshape(P, n)
        one.close()
        assert (ret[0] == ret[1]).all() and (ret[4, ::2] == ret[2, ::2]).all() and (ret[3, :10] == ret[0, :10]).all() and np.unique(ret).size > n
        unsafe = np.zeros(n, bool)
        if variant == 'safe':                                          # cem_reduce_kernel's own flags: where its score moves with the threshold
            lax, strict = (_planner(pb, variant, t, N=E, H=1, P=P, E=E, k=1, I=1) for t in (NEVER, thr))
            unsafe = _np(lax.compute_objective(traj)) != _np(strict.compute_objective(traj))
            print('planted ties, safe: %d of %d candidates unsafe' % (unsafe.sum(), n))
            lax.close(); strict.close()
        pl = _planner(pb, variant, thr, N=E, H=1, P=P, E=E, k=1, I=1)
        mean = _np(pl.compute_objective(traj))
        for m in rc.tail_ms(P):
            pl.set_particle_objective('lower_tail', m)
            want = rc.lower_tail_values(ret, m) - np.where(unsafe, np.float32(1.0), np.float32(0.0)) * np.float32(100.0)
            np.testing.assert_array_equal(_np(pl.compute_objective(traj)), want, err_msg='%s m = %d' % (variant, m))
        pl.set_particle_objective('mean')
        np.testing.assert_array_equal(_np(pl.compute_objective(traj)), mean)
        pl.close()


# ------------------------------------------------------------------------------------------------- 3: whole plans
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_whole_plan_graph_eager_and_stepwise_agree(variant):
    torch = _torch()
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    k, I = 13, 4
    pb = rc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1, noise=0.03)
    pg, pe, ps = (_planner(pb, variant, thr, worst=2, use_graph=g, **kw) for g in (True, False, False))
    for call in range(3):
        ag, sg, ig = pg.plan(pb['state'], seed=21, call=call)
        ae, se, ie = pe.plan(pb['state'], seed=21, call=call)
        ps.plan_begin(pb['state'], seed=21, call=call)
        for it in range(I):
            ps.plan_rollout(it)
            ps.plan_select(it)
        a2, s2, i2 = ps.plan_end()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ag, ae); np.testing.assert_array_equal(ag, a2)
        assert sg == se == s2 and ig == ie == i2 == I
        for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns'):
            assert torch.equal(getattr(pg, view)(), getattr(ps, view)()) and torch.equal(getattr(pe, view)(), getattr(ps, view)()), (view, call)
        np.testing.assert_array_equal(_np(pg.scores_local()), _want(pg, 2, variant == 'safe', thr)[0])
    assert (pg.graph_status(), pe.graph_status()) == ('graph', 'eager')
    assert pg.particle_objective() == ('lower_tail', 2) and pg.launches_per_iteration() == 3
    for p in (pg, pe, ps):
        p.close()


# ------------------------------------------------------------------------------------------------- 4: the other rollout families
@pytest.mark.parametrize('how', ['bf16x3', 'tanh256'])
def test_scores_behind_the_other_rollout_kernels(how):
    """All rollout families write the same returns / cost arrays: the split-product and the wide kernel too."""
    _torch()
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    pb = rc.problem(E=E) if how == 'bf16x3' else rc.problem(E=E, units=256, activation='tanh')
    pl = _planner(pb, 'safe', thr, worst=2, N=N, H=H, P=P, E=E, k=13, I=1, **(dict(precision='bf16x3') if how == 'bf16x3' else {}))
    assert (pl.cfg.precision, pl.cfg.units, pl.cfg.activation) == (('bf16x3', 32, 'relu') if how == 'bf16x3' else ('fp32', 256, 'tanh'))
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=rc.NOISE_SEED)
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    pl.plan_rollout(0)
    want, unsafe = _want(pl, 2, True, thr)
    np.testing.assert_array_equal(_np(pl.scores_local()), want)
    assert np.unique(want).size > N // 2
    pl.plan_select(0)
    pl.plan_end(eps_out=np.zeros(A, np.float32))
    pl.close()


# ------------------------------------------------------------------------------------------------- 5: batch handles, warm start
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_batch_rows_equal_their_single_plans(variant):
    torch = _torch()
    from ethz_safe_learning_amd import BatchCemPlanner
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    k, I, mb, n = 13, 3, 4, 3
    pb = rc.problem(E=E)
    _, pcfg = rc.configs(pb, worst=2, variant=variant, post=thr, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1, noise=0.02, use_graph=True)
    single = hp.make_planner(pb, pcfg)
    batch = BatchCemPlanner(pcfg, mb)
    batch.set_weights(pb['weights']); batch.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    assert batch.particle_objective() == ('lower_tail', 2)
    rng = np.random.default_rng(4)
    states = np.repeat(pb['state'][None], n, 0)
    states[1:] += rng.normal(0, 0.05, states[1:].shape).astype(np.float32)
    calls = np.array([7, 1 << 33, 9], np.uint64)
    lay = batch.layout

    def slices():
        batch.synchronize()
        v = dict(scores=batch._view(lay.scores_local, mb * N, torch.float32).view(mb, N), elite=batch._view(lay.elite_idx, mb * k, torch.int32).view(mb, k),
                 returns=batch._view(lay.returns, mb * P * N, torch.float32).view(mb, P, N), musig=batch._view(lay.mu_sigma, mb * 2 * H * A, torch.float32).view(mb, 2, H, A))
        if variant == 'safe':
            v['costs'] = batch._view(lay.costs, mb * H * P * N, torch.uint8).view(mb, H, P, N)
        return {key: _np(t) for key, t in v.items()}
    before = slices()
    acts, scores, iters = batch.plan_batch(states, seed=3, calls=calls)
    after = slices()
    assert batch.graph_status() == 'graph' and batch.launches_per_iteration() == 3
    for b in range(n):
        a1, s1, i1 = single.plan(states[b], seed=3, call=int(calls[b]))
        np.testing.assert_array_equal(acts[b], a1)
        assert scores[b] == s1 and iters[b] == i1
        np.testing.assert_array_equal(after['scores'][b], _np(single.scores_local()))
        np.testing.assert_array_equal(after['returns'][b], _np(single.returns()))
        np.testing.assert_array_equal(after['scores'][b], rc.scores(after['returns'][b], 2, after.get('costs', [None] * mb)[b], thr))
        np.testing.assert_array_equal(after['musig'][b], _np(single.mu_sigma()))
        np.testing.assert_array_equal(np.sort(after['elite'][b]), np.sort(_np(single.elite_idx())))
    for key in ('scores', 'elite', 'returns'):                          # the fourth problem sat out: its slices are as they were
        np.testing.assert_array_equal(after[key][n:], before[key][n:], err_msg=key)
    single.close(); batch.close()


def test_warm_started_plans_graph_equals_eager():
    _torch()
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    pb = rc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=3, noise=0.02)
    pg, pe = (_planner(pb, 'cem', thr, worst=1, use_graph=g, **kw) for g in (True, False))
    for p in (pg, pe):
        p.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
        p.set_init_mode('shift')
    for call in range(3):
        (ag, sg, _), (ae, se, _) = pg.plan(pb['state'], seed=2, call=call), pe.plan(pb['state'], seed=2, call=call)
        np.testing.assert_array_equal(ag, ae)
        assert sg == se
        np.testing.assert_array_equal(_np(pg.scores_local()), rc.scores(_np(pg.returns()), 1))
        np.testing.assert_array_equal(_np(pg.mu_sigma()), _np(pe.mu_sigma()))
    pg.close(); pe.close()


# ------------------------------------------------------------------------------------------------- 6: switching and refusals
def test_switching_back_to_the_mean_gives_a_default_handles_bits():
    torch = _torch()
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    pb = rc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=3, noise=0.02, use_graph=True)
    pl, fresh = _planner(pb, 'cem', thr, **kw), _planner(pb, 'cem', thr, **kw)
    assert pl.launches_per_iteration() == 2
    pl.plan(pb['state'], seed=6, call=0)                               # a captured default graph exists before the switch
    pl.set_particle_objective('lower_tail', 1)
    assert pl.launches_per_iteration() == 3 and pl.graph_status() == 'eager'
    pl.plan(pb['state'], seed=6, call=1)
    assert pl.graph_status() == 'graph'
    np.testing.assert_array_equal(_np(pl.scores_local()), rc.scores(_np(pl.returns()), 1))
    pl.set_particle_objective('mean')
    assert pl.launches_per_iteration() == 2 and pl.particle_objective() == ('mean', 0)
    a_m, s_m, i_m = pl.plan(pb['state'], seed=6, call=1)
    a_f, s_f, i_f = fresh.plan(pb['state'], seed=6, call=1)
    np.testing.assert_array_equal(a_m, a_f)
    assert s_m == s_f and i_m == i_f
    for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns'):
        assert torch.equal(getattr(pl, view)(), getattr(fresh, view)()), view
    pl.close(); fresh.close()


def _status(fn, *a):
    from ethz_safe_learning_amd._capi import CemError
    with pytest.raises(CemError) as e:
        fn(*a)
    return e.value.status


def test_refusals():
    _torch()
    P, N, H, E, thr = rc.SHAPES['p5_n130_h8']
    pb = rc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=2)
    cost = _planner(pb, 'cost', thr, **kw)
    assert _status(cost.set_particle_objective, 'lower_tail', 1) == UNSUPPORTED
    cost.set_particle_objective('mean')                                # the default is always accepted
    cost.close()
    with pytest.raises(Exception):
        _planner(pb, 'cost', thr, worst=1, **kw)
    pl = _planner(pb, 'safe', thr, **kw)
    assert _status(pl.set_particle_objective, 'lower_tail', 0) == INVALID_ARG
    assert _status(pl.set_particle_objective, 'lower_tail', P + 1) == INVALID_ARG
    assert pl.lib.cem_planner_set_particle_objective(pl.h, 2, 1) == INVALID_ARG
    pl.set_particle_objective('lower_tail', P)
    pl.plan_begin(pb['state'], seed=1, call=0)
    assert _status(pl.set_particle_objective, 'mean') == STATE
    assert _status(pl.set_particle_objective, 'lower_tail', 1) == STATE
    for it in range(2):
        pl.plan_rollout(it); pl.plan_select(it)
    pl.plan_end()
    assert pl.particle_objective() == ('lower_tail', P)                 # every refusal left the setting alone
    pl.set_particle_objective('mean')
    pl.close()


# ------------------------------------------------------------------------------------------------- 7: the policies
def _parts(name):
    from tests.test_simba_api import make_agent_parts, trained_like
    env, model, pol = make_agent_parts(name, seed=3)
    trained_like(model, np.random.default_rng(0))
    return env, model, pol


def _state():
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    return PointGoalEnv(seed=0).reset().astype(np.float32)


def test_cem_mpc_risk_level_plans_on_the_worst_particle():
    torch = _torch()
    from ethz_safe_learning_amd import CemPlanner
    from ethz_safe_learning_amd.planner import planner_cache_info
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from tests.test_simba_api import POLICIES_YAML
    env, model, plain = _parts('cem_mpc')
    st = _state()
    plain.build(); plain._planner._call = 50
    a_plain = plain.generate_action(st)
    n_handles = planner_cache_info()['size']
    none = CemMpc(model=model, environment=env, risk_level=None, **dict(POLICIES_YAML['cem_mpc']))
    none.build(); none._planner._call = 50
    assert none._planner is plain._planner and planner_cache_info()['size'] == n_handles and none.worst_particles == 0
    np.testing.assert_array_equal(none.generate_action(st), a_plain)
    assert none._planner.particle_objective() == ('mean', 0)
    risk = CemMpc(model=model, environment=env, risk_level=0.2, **dict(POLICIES_YAML['cem_mpc']))
    assert risk.particles == 5 and risk.worst_particles == 1
    risk.build(); risk._planner._call = 50
    assert risk._planner is not plain._planner and risk._planner.particle_objective() == ('lower_tail', 1)
    a_risk = risk.generate_action(st)
    ref = CemPlanner(dataclasses.replace(plain.planner_config(), worst_particles=1))       # a handle of its own, not the cache's
    ref.staged = None
    risk._sync_model(ref)
    a_ref, s_ref, _ = ref.plan(st, seed=risk.seed, call=50)
    np.testing.assert_array_equal(a_risk, a_ref)
    assert risk.last_score == s_ref
    np.testing.assert_array_equal(_np(risk._planner.scores_local()), rc.scores(_np(risk._planner.returns()), 1))
    # generate_actions: the batch handle carries the setting; compute_objective aggregates the same way
    rows = risk.generate_actions(np.stack([st, st]))
    assert risk._batch_planners[2].particle_objective() == ('lower_tail', 1) and rows.shape == (2, 2)
    traj = np.random.default_rng(1).uniform(0.05, 0.95, (5 * 6, 4, model.observation_space_dim)).astype(np.float32)
    per_row = CemMpc(model=model, environment=env, **dict(POLICIES_YAML['cem_mpc'], particles=1)).compute_objective(traj).reshape(5, 6)
    np.testing.assert_array_equal(risk.compute_objective(traj), rc.lower_tail_values(per_row, 1))
    ref.close()


def test_safe_cem_mpc_risk_level_leaves_the_cost_plans_on_the_mean():
    _torch()
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    from tests.test_simba_api import POLICIES_YAML
    env, model, plain = _parts('safe_cem_mpc')
    st = _state()
    risk = SafeCemMpc(model=model, environment=env, risk_level=0.2, **dict(POLICIES_YAML['safe_cem_mpc']))
    assert risk.worst_particles == 9 and risk.planner_config().worst_particles == 9 and risk.cost_planner_config().worst_particles == 0
    a = risk.generate_action(st)
    assert risk._planner.particle_objective() == ('lower_tail', 9) and a.shape == (2,)
    thr = risk.posterior_mean_threashold
    np.testing.assert_array_equal(_np(risk._planner.scores_local()),
                                  rc.scores(_np(risk._planner.returns()), 9, _np(risk._planner.costs()), thr))
    np.testing.assert_array_equal(risk.optimize_for_safety(st, call=4), plain.optimize_for_safety(st, call=4))
    assert risk._cost_planner is plain._cost_planner and risk._cost_planner.particle_objective() == ('mean', 0)
