"""Budget-constrained planning on the device (cem_planner_set_constraint, CEM_CONSTRAINT_BUDGET; csrc/cem_score.h) against its NumPy
restatement (tests/constrained_cases.py).

Every expected score is computed from the handle's OWN returns() and costs() of the same rollout: integer sums, one division, one
comparison, cem_reduce_kernel's sequential mean and an exact encoding have one right answer, so every score comparison is
assert_array_equal and no tolerance exists to be measured."""
import dataclasses

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import constrained_cases as kc
from tests import helpers as hp
from tests import risk_cases as rc

pytestmark = pytest.mark.gpu

O, A = 60, 2                                     # cost_cases.problem
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7        # enum cem_status
INF = float('inf')


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _planner(pb, constraint='budget', worst_cost=0, **kw):
    _, pcfg = kc.configs(pb, constraint=constraint, worst_cost=worst_cost, **kw)
    return hp.make_planner(pb, pcfg)


def _want(pl, m_c, budget):
    """The restatement on what the handle's last rollout left."""
    ret, costs = _np(pl.returns()), _np(pl.costs())
    P, N = ret.shape
    return kc.scores(ret, costs, P, N, m_c, budget), kc.cost_stats(costs, P, N, m_c)


def _first_iteration(pl, pb, budget, m_c, k, **begin):
    """One stepwise iteration at `budget` -> (scores, cstat, elites, best score of the plan); everything compared with the restatement."""
    pl.set_cost_budget(budget)
    pl.plan_begin(pb['state'], **begin)
    pl.plan_rollout(0)
    got, cst = _np(pl.scores_local()), pl.constraint_costs()
    want, want_c = _want(pl, m_c, budget)
    np.testing.assert_array_equal(cst, want_c)
    np.testing.assert_array_equal(got, want)
    pl.plan_select(0)
    elite = np.sort(_np(pl.elite_idx()))
    np.testing.assert_array_equal(elite, kc.top_k(got, k))
    for it in range(1, pl.cfg.iterations):
        pl.plan_rollout(it); pl.plan_select(it)
    _, best, _ = pl.plan_end(eps_out=np.zeros(A, np.float32))
    return got, cst, elite, best


def _median_budget(pl, pb, m_c, **begin):
    """The median of the restated C of the first iteration (the budget plays no part in the rollout)."""
    pl.set_cost_budget(INF)
    pl.plan_begin(pb['state'], **begin)
    pl.plan_rollout(0)
    ret, costs = _np(pl.returns()), _np(pl.costs())
    np.testing.assert_array_equal(_np(pl.scores_local()), kc.mean_returns(ret))          # +inf: everything is feasible
    pl.plan_select(0)
    for it in range(1, pl.cfg.iterations):
        pl.plan_rollout(it); pl.plan_select(it)
    pl.plan_end(eps_out=np.zeros(A, np.float32))
    return float(np.median(kc.cost_stats(costs, ret.shape[0], ret.shape[1], m_c)))


# ------------------------------------------------------------------------------------------------- 1: stepwise scores and elites
@pytest.mark.parametrize('case', list(kc.SHAPES))
def test_stepwise_scores_costs_and_elites_equal_the_restatement(case):
    _torch()
    P, N, H, E, size_frac = kc.SHAPES[case]
    k = 9
    pb = kc.problem(E=E, size_frac=size_frac)
    pl = _planner(pb, N=N, H=H, P=P, E=E, k=k, I=1)
    assert pl.constraint() == ('budget', P) and pl.launches_per_iteration() == 3
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=kc.NOISE_SEED)
    for m_c in rc.tail_ms(P):
        pl.set_constraint('budget', m_c)
        assert pl.constraint() == ('budget', m_c)
        budget = _median_budget(pl, pb, m_c, eps_act=ea, eps_model=em)
        got, cst, elite, best = _first_iteration(pl, pb, budget, m_c, k, eps_act=ea, eps_model=em)
        feas = cst <= np.float32(budget)
        print('%s m_c = %d: budget %.4f, %d of %d feasible, C %.3f .. %.3f' % (case, m_c, budget, feas.sum(), N, cst.min(), cst.max()))
        assert feas.any() and (~feas).any(), 'the median budget should split the candidates of this case'
        np.testing.assert_array_equal(got > np.float32(-2.0 ** 100), feas)
        ret, costs = _np(pl.returns()), _np(pl.costs())
        np.testing.assert_array_equal(elite, kc.constrained_elites(ret, costs, P, N, m_c, budget, k))
        assert best == got.max()
    pl.close()


# ------------------------------------------------------------------------------------------------- 2: budget +inf
@pytest.mark.parametrize('graph', [True, False])
def test_an_infinite_budget_plans_like_a_filter_that_never_fires(graph):
    torch = _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=4, smoothing=0.1, noise=0.03, use_graph=graph)
    pl = _planner(pb, **kw)                                            # the default budget IS +inf
    ref = _planner(pb, constraint='beta', post=1e30, **kw)             # no posterior mean exceeds 1e30
    for call in range(3):
        a, s, i = pl.plan(pb['state'], seed=4, call=call)
        ar, sr, ir = ref.plan(pb['state'], seed=4, call=call)
        np.testing.assert_array_equal(a, ar)
        assert s == sr and i == ir
        for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns', 'costs'):
            assert torch.equal(getattr(pl, view)(), getattr(ref, view)()), (view, call)
    assert pl.graph_status() == ref.graph_status() == ('graph' if graph else 'eager')
    assert _np(pl.costs()).max() >= 1                                  # there were costs to ignore
    pl.close(); ref.close()


# ------------------------------------------------------------------------------------------------- 3: budget -1
@pytest.mark.parametrize('worst_cost', [0, 2])
def test_a_negative_budget_ranks_by_ascending_cost(worst_cost):
    _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    k, m_c = 13, worst_cost or P
    pb = kc.problem(E=E, size_frac=size_frac)
    pl = _planner(pb, worst_cost=worst_cost, N=N, H=H, P=P, E=E, k=k, I=1)
    got, cst, elite, best = _first_iteration(pl, pb, -1.0, m_c, k, seed=3, call=1)
    T = kc.totals(_np(pl.costs()), P, N, m_c)
    assert [kc.decode(s) for s in got] == [(False, int(t)) for t in T]
    np.testing.assert_array_equal(elite, np.sort(np.argsort(T, kind='stable')[:k]))      # the k smallest T, ties to the lowest index
    assert (T == np.sort(T)[k - 1]).sum() > 1 or np.unique(T).size < N                   # (integers over 130 candidates: there are ties)
    assert kc.decode(best) == (False, int(T.min()))
    from ethz_safe_learning_amd.planner import decode_constrained_score
    assert decode_constrained_score(best) == (False, int(T.min()))
    pl.close()


# ------------------------------------------------------------------------------------------------- 4: planted trajectories
def test_planted_trajectories_through_compute_objective():
    _torch()
    P, n, H = kc.HAND_P, kc.HAND_N, kc.HAND_H
    pb = dict(kc.problem(E=3), scorer=kc.HAND_SP)
    traj = kc.hand_trajectory(O)
    kw = dict(N=3, H=1, P=P, E=3, k=1, I=1)
    # the per-row returns: a one-particle handle under a Beta filter that never fires scores every row by itself ((0 + r) / 1 = r)
    one = _planner(pb, constraint='beta', post=1e30, **dict(kw, P=1))
    ret = _np(one.compute_objective(traj)).reshape(P, n)
    one.close()
    assert np.unique(ret).size > 1
    pl = _planner(pb, **kw)
    pl.set_cost_budget(kc.HAND_BUDGET)
    for m_c in (3, 2, 1):
        pl.set_constraint('budget', m_c)
        got = _np(pl.compute_objective(traj))
        np.testing.assert_array_equal(got, kc.scores(ret, kc.HAND_COSTS, P, n, m_c, kc.HAND_BUDGET), err_msg='m_c = %d' % m_c)
        np.testing.assert_array_equal(pl.constraint_costs(n=n), kc.HAND_TOTALS[m_c].astype(np.float32) / np.float32(m_c))
        feas = got > np.float32(-2.0 ** 100)
        np.testing.assert_array_equal(feas, kc.HAND_SCORES[m_c] > np.float32(-2.0 ** 100))
        np.testing.assert_array_equal(got[~feas], kc.HAND_SCORES[m_c][~feas])             # the encoded totals as written by hand
        assert feas[0]                                                 # exactly on the budget: feasible
    pl.set_constraint('budget', 0)                                     # candidate 1: feasible on the mean ...
    assert kc.decode(_np(pl.compute_objective(traj))[1]) == (True, None)
    pl.set_constraint('budget', 1)                                     # ... not on its worst particle
    assert kc.decode(_np(pl.compute_objective(traj))[1]) == (False, 3)
    pl.set_cost_budget(np.nextafter(np.float32(1), np.float32(0)))     # a hair below: candidate 0 is out
    assert kc.decode(_np(pl.compute_objective(traj))[0]) == (False, 1)
    pl.close()


# ------------------------------------------------------------------------------------------------- 5: whole plans
@pytest.mark.parametrize('case', ['p5_n130_h8', 'p17_n130_h33'])
def test_whole_plan_graph_eager_stepwise_and_the_restated_loop_agree(case):
    torch = _torch()
    P, N, H, E, size_frac = kc.SHAPES[case]
    k, I, m_c = 13, 3, 2
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(worst_cost=m_c, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1)
    pg, pe, ps = (_planner(pb, use_graph=g, **kw) for g in (True, False, False))
    ocfg, _ = kc.configs(pb, **{x: v for x, v in kw.items() if x != 'worst_cost'})
    budget = _median_budget(ps, pb, m_c, seed=21, call=0)
    for p in (pg, pe, ps):
        p.set_cost_budget(budget)
    for call in range(2):
        ag, sg, ig = pg.plan(pb['state'], seed=21, call=call)
        ae, se, ie = pe.plan(pb['state'], seed=21, call=call)
        ea, _, eo = ps.fill_noise(seed=21, call=call)
        ps.plan_begin(pb['state'], seed=21, call=call)
        best, best_score, dev_scores, n_feas = np.zeros(A, np.float32), np.float32(-np.inf), [], []
        for it in range(I):                                            # the restated loop, fed the device's own scores / actions / mu / sigma
            ps.plan_rollout(it)
            scores, actions, ms0 = _np(ps.scores_local()), _np(ps.actions()), _np(ps.mu_sigma())
            np.testing.assert_array_equal(scores, _want(ps, m_c, budget)[0])
            dev_scores.append(scores); n_feas.append(int((scores > np.float32(-2.0 ** 100)).sum()))
            _, _, best, best_score, elite, _ = o.select_and_refit(scores, actions, ms0[0], ms0[1], best, best_score, ocfg)
            ps.plan_select(it)
            np.testing.assert_array_equal(np.sort(_np(ps.elite_idx())), elite)
        a2, s2, i2 = ps.plan_end()
        torch.cuda.synchronize()
        print('%s call %d: feasible per iteration %s of %d' % (case, call, n_feas, N))
        np.testing.assert_array_equal(ag, ae); np.testing.assert_array_equal(ag, a2)
        assert sg == se == s2 == best_score and ig == ie == i2 == I
        np.testing.assert_array_equal(a2, best + _np(eo) * np.float32(0.0))
        for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns', 'costs'):
            assert torch.equal(getattr(pg, view)(), getattr(ps, view)()) and torch.equal(getattr(pe, view)(), getattr(ps, view)()), (view, call)
        np.testing.assert_array_equal(pg.constraint_costs(), ps.constraint_costs())
        # the loop of constrained_cases.plan on those scores: the same best score and count (its actions are its own samples)
        _, s3, i3 = kc.plan(pb['state'], pb['low'], pb['high'], _np(ea), np.zeros(A, np.float32), ocfg, lambda it, actions: dev_scores[it])
        assert s3 == s2 and i3 == I
        if call == 0:
            assert 0 < n_feas[0] < N
    assert (pg.graph_status(), pe.graph_status()) == ('graph', 'eager') and pg.launches_per_iteration() == 3
    for p in (pg, pe, ps):
        p.close()


# ------------------------------------------------------------------------------------------------- 6: the budget moves, the graph stays
def test_changing_the_budget_does_not_recapture():
    torch = _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=3, smoothing=0.1, noise=0.02, use_graph=True)
    pl, fresh = _planner(pb, **kw), _planner(pb, **kw)
    probe = _planner(pb, **dict(kw, use_graph=False))
    b_med = _median_budget(probe, pb, P, seed=6, call=5)
    probe.close()
    a_inf, s_inf, _ = pl.plan(pb['state'], seed=6, call=5)             # budget A = +inf, captured
    assert pl.graph_status() == 'graph'
    pl.set_cost_budget(b_med)
    assert pl.graph_status() == 'graph'                                # nothing dropped
    a_b, s_b, i_b = pl.plan(pb['state'], seed=6, call=5)
    fresh.set_cost_budget(b_med)
    a_f, s_f, i_f = fresh.plan(pb['state'], seed=6, call=5)
    np.testing.assert_array_equal(a_b, a_f)
    assert s_b == s_f and i_b == i_f
    for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions'):
        assert torch.equal(getattr(pl, view)(), getattr(fresh, view)()), view
    np.testing.assert_array_equal(_np(pl.scores_local()), _want(pl, P, b_med)[0])
    pl.set_cost_budget(INF)                                            # ... and back
    a_again, s_again, _ = pl.plan(pb['state'], seed=6, call=5)
    np.testing.assert_array_equal(a_again, a_inf)
    assert s_again == s_inf and pl.graph_status() == 'graph'
    pl.close(); fresh.close()


def test_batch_rows_carry_their_own_budgets():
    _torch()
    from ethz_safe_learning_amd import BatchCemPlanner
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    k, I, mb, n = 13, 3, 4, 3
    pb = kc.problem(E=E, size_frac=size_frac)
    _, pcfg = kc.configs(pb, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1, noise=0.02, use_graph=True)
    single = hp.make_planner(pb, pcfg)
    batch = BatchCemPlanner(pcfg, mb)
    batch.set_weights(pb['weights']); batch.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    assert batch.constraint() == ('budget', P)
    rng = np.random.default_rng(4)
    states = np.repeat(pb['state'][None], n, 0)
    states[1:] += rng.normal(0, 0.05, states[1:].shape).astype(np.float32)
    calls = np.array([7, 1 << 33, 9], np.uint64)
    b_med = _median_budget(single, pb, P, seed=3, call=7)
    for budgets in ([INF, -1.0, INF], [b_med, -INF, INF]):
        batch.set_cost_budget(budgets)
        acts, scores, iters = batch.plan_batch(states, seed=3, calls=calls)
        assert batch.graph_status() == 'graph'
        for b in range(n):
            single.set_cost_budget(budgets[b])
            a1, s1, i1 = single.plan(states[b], seed=3, call=int(calls[b]))
            np.testing.assert_array_equal(acts[b], a1)
            assert scores[b] == s1 and iters[b] == i1
            np.testing.assert_array_equal(batch.constraint_costs(problem=b), single.constraint_costs())
        feas = scores > np.float32(-2.0 ** 100)
        assert [bool(f) for f in feas] == [bud > 0 for bud in budgets]                  # (row 0's first iteration has candidates at or below its median)
    batch.set_cost_budget(b_med)                                       # one value: every row
    acts, scores, iters = batch.plan_batch(states, seed=3, calls=calls)
    single.set_cost_budget(b_med)
    for b in range(n):
        a1, s1, _ = single.plan(states[b], seed=3, call=int(calls[b]))
        np.testing.assert_array_equal(acts[b], a1)
        assert scores[b] == s1
    single.close(); batch.close()


# ------------------------------------------------------------------------------------------------- 7: the other paths
@pytest.mark.parametrize('how', ['bf16x3', 'tanh256'])
def test_scores_behind_the_other_rollout_kernels(how):
    """All rollout families write the same returns / cost arrays: the split-product and the wide kernel too."""
    _torch()
    P, N, H, E, k, m_c = 5, 130, 8, 5, 13, 2
    pb = kc.problem(E=E, size_frac=0.7) if how == 'bf16x3' else kc.problem(E=E, size_frac=0.7, units=256, activation='tanh')
    pl = _planner(pb, worst_cost=m_c, N=N, H=H, P=P, E=E, k=k, I=1, **(dict(precision='bf16x3') if how == 'bf16x3' else {}))
    assert (pl.cfg.precision, pl.cfg.units, pl.cfg.activation) == (('bf16x3', 128, 'relu') if how == 'bf16x3' else ('fp32', 256, 'tanh'))
    budget = _median_budget(pl, pb, m_c, seed=2, call=0)
    got, cst, _, _ = _first_iteration(pl, pb, budget, m_c, k, seed=2, call=0)
    feas = cst <= np.float32(budget)
    print('%s: budget %.3f, %d of %d feasible' % (how, budget, feas.sum(), N))
    assert feas.any() and (~feas).any(), 'the median budget should split the candidates behind this rollout kernel too'
    pl.close()


def test_a_population_for_the_multi_workgroup_select():
    """N just above 24 000: the reduce clears the select's histogram / barrier words and the multi-workgroup select ranks the encoded scores."""
    _torch()
    P, N, H, E, k, m_c = 2, 24010, 3, 5, 50, 1
    pb = kc.problem(E=E, size_frac=0.9)
    pl = _planner(pb, worst_cost=m_c, N=N, H=H, P=P, E=E, k=k, I=2)
    assert pl.select_mode() in (2, 3)
    budget = _median_budget(pl, pb, m_c, seed=8, call=0)
    got, cst, elite, best = _first_iteration(pl, pb, budget, m_c, k, seed=8, call=0)
    feas = cst <= np.float32(budget)
    print('N = %d: budget %.3f, %d feasible, select mode %d' % (N, budget, feas.sum(), pl.select_mode()))
    assert feas.any() and (~feas).any()
    got2, _, elite2, _ = _first_iteration(pl, pb, -1.0, m_c, k, seed=8, call=0)        # nothing feasible: k of the cheapest, lowest indices first
    T = kc.totals(_np(pl.costs()), P, N, m_c)
    assert (got2 <= np.float32(-2.0 ** 100)).all() and np.unique(T).size <= H + 1
    pl.close()


def test_warm_started_plans_graph_equals_eager():
    _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=3, noise=0.02)
    pg, pe = (_planner(pb, use_graph=g, **kw) for g in (True, False))
    probe = _planner(pb, **kw)
    budget = _median_budget(probe, pb, P, seed=2, call=0)
    probe.close()
    for p in (pg, pe):
        p.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
        p.set_init_mode('shift')
        p.set_cost_budget(budget)
    for call in range(3):
        (ag, sg, _), (ae, se, _) = pg.plan(pb['state'], seed=2, call=call), pe.plan(pb['state'], seed=2, call=call)
        np.testing.assert_array_equal(ag, ae)
        assert sg == se
        np.testing.assert_array_equal(_np(pg.scores_local()), _want(pg, P, budget)[0])
        np.testing.assert_array_equal(_np(pg.mu_sigma()), _np(pe.mu_sigma()))
    assert pg.carry()[2] and pg.graph_status() == 'graph'
    pg.close(); pe.close()


def test_constraint_costs_follow_a_replayed_graph_after_the_objective_op():
    """graph plan, compute_objective, replayed graph plan: constraint_costs is the last PLAN's array, not the op's."""
    _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    pl = _planner(pb, N=N, H=H, P=P, E=E, k=13, I=2, use_graph=True)
    pl.plan(pb['state'], seed=9, call=0)
    assert pl.graph_status() == 'graph'
    np.testing.assert_array_equal(pl.constraint_costs(), _want(pl, P, INF)[1])
    traj = np.random.default_rng(1).uniform(0.05, 0.95, (P * 7, 4, O)).astype(np.float32)     # 7 candidates, 3 steps: another array altogether
    pl.compute_objective(traj)
    op_costs = pl.constraint_costs(n=7)
    assert op_costs.shape == (7,) and _status(pl.constraint_costs, 0, N) == INVALID_ARG      # the op's array holds 7 candidates
    pl.plan(pb['state'], seed=9, call=1)                               # replayed: no enqueue function runs
    assert pl.graph_status() == 'graph'
    got = pl.constraint_costs()
    np.testing.assert_array_equal(got, _want(pl, P, INF)[1])
    assert got.shape == (N,) and np.unique(got).size > 1
    pl.close()


# ------------------------------------------------------------------------------------------------- 8: back to the Beta filter
def test_switching_back_to_beta_gives_a_default_handles_bits():
    torch = _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=3, noise=0.02, use_graph=True, post=0.3)
    pl, fresh = _planner(pb, constraint='beta', **kw), _planner(pb, constraint='beta', **kw)
    assert pl.constraint() == ('beta', 0) and pl.launches_per_iteration() == 3
    pl.plan(pb['state'], seed=6, call=0)                               # a captured default graph exists before the switch
    pl.set_constraint('budget', 2)
    assert pl.launches_per_iteration() == 3 and pl.graph_status() == 'eager'
    pl.set_cost_budget(-1.0)
    _, s, _ = pl.plan(pb['state'], seed=6, call=1)
    assert pl.graph_status() == 'graph' and kc.decode(s)[0] is False
    pl.set_constraint('beta')
    assert pl.constraint() == ('beta', 0) and pl.graph_status() == 'eager'
    a_m, s_m, i_m = pl.plan(pb['state'], seed=6, call=1)
    a_f, s_f, i_f = fresh.plan(pb['state'], seed=6, call=1)
    np.testing.assert_array_equal(a_m, a_f)
    assert s_m == s_f and i_m == i_f
    for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns', 'costs'):
        assert torch.equal(getattr(pl, view)(), getattr(fresh, view)()), view
    pl.close(); fresh.close()


# ------------------------------------------------------------------------------------------------- 9: refusals
def _status(fn, *a, **kw):
    from ethz_safe_learning_amd._capi import CemError
    with pytest.raises(CemError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals():
    _torch()
    P, N, H, E, size_frac = kc.SHAPES['p5_n130_h8']
    pb = kc.problem(E=E, size_frac=size_frac)
    kw = dict(N=N, H=H, P=P, E=E, k=13, I=2)
    for variant in ('cem', 'cost'):                                    # BUDGET needs the SAFE rollout's cost bytes
        _, pcfg = hp.configs(pb, variant=variant, **kw)
        other = hp.make_planner(pb, pcfg)
        assert _status(other.set_constraint, 'budget', 0) == UNSUPPORTED
        other.set_constraint('beta')                                   # the default is always accepted
        assert other.constraint() == ('beta', 0)
        assert _status(other.constraint_costs) == STATE                # no constrained reduce has run
        other.close()
        with pytest.raises(Exception):
            hp.make_planner(pb, dataclasses.replace(pcfg, constraint='budget'))
    pl = _planner(pb, constraint='beta', **kw)
    assert _status(pl.set_constraint, 'budget', -1) == INVALID_ARG
    assert _status(pl.set_constraint, 'budget', P + 1) == INVALID_ARG
    assert pl.lib.cem_planner_set_constraint(pl.h, 2, 0) == INVALID_ARG
    assert _status(pl.set_cost_budget, float('nan')) == INVALID_ARG
    assert _status(pl.set_cost_budget, [1.0, 2.0]) == INVALID_ARG      # two rows on a single-state handle
    assert pl.lib.cem_planner_set_cost_budget(pl.h, None, 1) == INVALID_ARG
    one = np.array([1.0], np.float32)
    assert pl.lib.cem_planner_set_cost_budget(pl.h, one.ctypes.data, 0) == INVALID_ARG
    assert pl.constraint() == ('beta', 0)
    # the lower tail of the returns and the budget exclude each other, in either order of setting
    pl.set_particle_objective('lower_tail', 2)
    assert _status(pl.set_constraint, 'budget', 0) == UNSUPPORTED
    pl.set_particle_objective('mean')
    pl.set_constraint('budget', P)
    assert _status(pl.set_particle_objective, 'lower_tail', 2) == UNSUPPORTED
    assert pl.constraint() == ('budget', P) and pl.particle_objective() == ('mean', 0)
    pl.set_cost_budget(-INF); pl.set_cost_budget(INF)                  # both infinities are budgets
    # inside a stepwise plan
    pl.plan_begin(pb['state'], seed=1, call=0)
    assert _status(pl.set_constraint, 'beta') == STATE
    assert _status(pl.set_constraint, 'budget', 1) == STATE
    assert _status(pl.set_cost_budget, 1.0) == STATE
    for it in range(2):
        pl.plan_rollout(it); pl.plan_select(it)
    pl.plan_end()
    assert pl.constraint() == ('budget', P)                            # every refusal left the setting alone
    assert _status(pl.constraint_costs, 1) == INVALID_ARG and _status(pl.constraint_costs, 0, N + 1) == INVALID_ARG
    pl.close()
    # the tail form holds eight particles a wave: 0 < m_c < P needs P <= 128; the mean form does not
    pbw = kc.problem(E=1)
    wide = _planner(pbw, constraint='beta', N=4, H=2, P=129, E=1, k=2, I=1)
    assert _status(wide.set_constraint, 'budget', 5) == UNSUPPORTED
    wide.set_constraint('budget', 0); wide.set_constraint('budget', 129)
    wide.close()
    # the encoding holds totals below 2^23: horizon x m_c x CEM_MAX_COST_KINDS
    deep = _planner(pbw, constraint='beta', N=1, H=32768, P=64, E=1, k=1, I=1)
    assert _status(deep.set_constraint, 'budget', 64) == UNSUPPORTED                    # 32768 * 64 * 4 = 2^23
    deep.set_constraint('budget', 63)
    deep.close()
    # world_size > 1
    _, shard = kc.configs(pb, constraint='beta', world_size=2, rank=0, **kw)
    sh = hp.make_planner(pb, shard)
    assert _status(sh.set_constraint, 'budget', 0) == UNSUPPORTED
    sh.close()


# ------------------------------------------------------------------------------------------------- 10: the policy
def _policy(seed=3, **extra):
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    env, model, pol = make_agent_parts('safe_cem_mpc', seed=seed)
    trained_like(model, np.random.default_rng(0))
    if extra:
        pol = SafeCemMpc(model=model, environment=env, **dict(POLICIES_YAML['safe_cem_mpc'], **extra))
    return env, model, pol


def _states(n):
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    return np.stack([PointGoalEnv(seed=s).reset() for s in range(n)]).astype(np.float32)


def test_policy_plans_within_its_budget_on_a_handle_of_its_own():
    _torch()
    from ethz_safe_learning_amd import CemPlanner
    st = _states(1)[0]
    _, _, plain = _policy()
    plain.build()
    _, _, pol = _policy(cost_budget=INF, cost_risk_level=0.2)
    assert pol.worst_cost_particles == 9 and pol.planner_config().constraint == 'budget' and pol.cost_planner_config().constraint == 'beta'
    pol.build(); pol._planner._call = 50
    assert pol._planner is not plain._planner and pol._planner.constraint() == ('budget', 9)
    a_inf = pol.generate_action(st)
    assert pol.last_feasible is True and pol.last_cost_total is None
    ref = CemPlanner(pol.planner_config())                            # a handle of its own, not the cache's
    ref.staged = None
    pol._sync_model(ref)
    a_ref, s_ref, _ = ref.plan(st, seed=pol.seed, call=50)
    np.testing.assert_array_equal(a_inf, a_ref)
    assert pol.last_score == s_ref
    pol.set_cost_budget(-1.0)                                          # between decisions: nothing can be feasible
    pol._planner._call = 50
    a_neg = pol.generate_action(st)
    assert pol.last_feasible is False and isinstance(pol.last_cost_total, int) and pol.last_cost_total >= 0
    assert pol._planner.graph_status() == 'graph'
    ret, costs = _np(pol._planner.returns()), _np(pol._planner.costs())
    np.testing.assert_array_equal(_np(pol._planner.scores_local()), kc.scores(ret, costs, 45, 500, 9, -1.0))
    ref.set_cost_budget(-1.0)
    a_ref, s_ref, _ = ref.plan(st, seed=pol.seed, call=50)
    np.testing.assert_array_equal(a_neg, a_ref)
    assert kc.decode(s_ref) == (False, pol.last_cost_total)
    ref.close()
    # a second policy of the shape has its own handle, hence its own budget
    _, _, other = _policy(cost_budget=3.0, cost_risk_level=0.2)
    other.build()
    assert other._planner is not pol._planner
    with pytest.raises(ValueError):
        plain.set_cost_budget(1.0)


def test_policy_rows_carry_budgets_and_recovery_replaces_an_infeasible_best():
    _torch()
    states = _states(3)
    _, _, pol = _policy(cost_budget=INF)
    pol.build_batch(3)._call = 50
    want = pol.generate_actions(states)
    assert pol.last_feasible.tolist() == [True, True, True] and list(pol.last_cost_total) == [None, None, None]
    pol.set_cost_budget([INF, -1.0, INF])
    pol.build_batch(3)._call = 50
    got = pol.generate_actions(states)
    assert pol.last_feasible.tolist() == [True, False, True] and pol.last_cost_total[1] >= 0 and pol.last_cost_total[0] is None
    np.testing.assert_array_equal(got[[0, 2]], want[[0, 2]])
    assert not np.array_equal(got[1], want[1])
    with pytest.raises(ValueError):
        pol.set_cost_budget([1.0, 2.0]); pol.generate_actions(states)
    # recover_below: an infeasible best lies below any threshold and is replaced by the optimize_for_safety action
    _, _, rec = _policy(cost_budget=-1.0, recover_below=-1e9)
    rec.build(); rec._planner._call = 50
    a = rec.generate_action(states[0])
    assert rec.last_feasible is False and rec.last_recovered is True
    np.testing.assert_array_equal(a, rec.optimize_for_safety(states[0], call=50))
    rec.set_cost_budget(INF)
    rec._planner._call = 50
    rec.generate_action(states[0])
    assert rec.last_feasible is True and rec.last_recovered is False


def test_policy_without_a_budget_is_the_parent_policy():
    _torch()
    from ethz_safe_learning_amd.planner import planner_cache_info
    st = _states(1)[0]
    _, _, plain = _policy()
    plain.build(); plain._planner._call = 50
    a_plain = plain.generate_action(st)
    n_handles = planner_cache_info()['size']
    _, _, none = _policy(cost_budget=None, cost_risk_level=None)
    none.build(); none._planner._call = 50
    assert none._planner is plain._planner and planner_cache_info()['size'] == n_handles
    np.testing.assert_array_equal(none.generate_action(st), a_plain)
    assert none.last_score == plain.last_score and none._planner.constraint() == ('beta', 0)
    assert none.last_feasible is None and none.last_cost_total is None
    from ethz_safe_learning_amd.planner import config_key
    assert config_key(none.planner_config()) == config_key(plain.planner_config())
