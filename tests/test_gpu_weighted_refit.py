"""The score-weighted refit (cem_planner_set_refit, CEM_REFIT_SOFTMAX) on the device, held to the float64 restatement of
tests/weighted_cases.py on the device's own actions and elite set (the bars of a select: tests/test_gpu_select_paths.py:78-79), and run
to run by bits.  The harness is test_gpu_select_paths's: H = 3, A = 2, P = E = 5, smoothing 0.25, one real rollout on fixed noise, the
case's vector written straight into the score buffer, one plan_select.

The kernel's depths (csrc/cem_refit_weighted.h), which the op cases straddle — in elites k, for a column block served by tpc parts
(H A = 6: tpc = 128; the first block of H A = 1030: tpc = 1):
  tpc                                    one row per part
  CEM_REFIT_KEEP x tpc = 4 tpc           the rows a thread gathers once and keeps in registers for both phases
  + CEM_REFIT_BATCH x tpc = 4 tpc each   every trip of the loop that gathers the rest again in each phase
  1024                                   one trip of the weight loop (an elite per thread)"""
import dataclasses

import numpy as np
import pytest

from tests import helpers as hp
from tests import weighted_cases as wc

pytestmark = pytest.mark.gpu

P, E, SMOOTHING = 5, 5, 0.25
F = np.float32
U = np.uint32
INVALID_ARG, STATE, UNSUPPORTED = 1, 7, 2
VARIANTS = ('cem', 'safe', 'cost')

_RUNS, _NOISE, _PB = {}, {}, {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _pb(A=2):
    if A not in _PB:
        _PB[A] = hp.make_problem(seed=42, act_dim=A)
    return _PB[A]


def _noise(I, N, H, A):
    key = (I, N, H, A)
    if key not in _NOISE:
        if len(_NOISE) > 3:
            _NOISE.clear()
        _NOISE[key] = hp.noise(I, N, H, A, P, 60, seed=1)
    return _NOISE[key]


def _pcfg(pb, variant, N, H, k, I=1, thr=-1.0, tau=None, **kw):
    _, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=SMOOTHING, variant='cem' if variant == 'cem' else 'safe', thr=thr, **kw)
    if variant == 'cost':
        pcfg = dataclasses.replace(pcfg, variant='cost')
    if tau is not None:
        pcfg = dataclasses.replace(pcfg, refit='softmax', refit_temperature=tau)
    return pcfg


def _select_once(name, variant, weighted, thr=-1.0, again=False):
    """One select of the case on a fresh handle -> what the device left (memoised)."""
    key = (name, variant, weighted, thr, again)
    if key in _RUNS:
        return _RUNS[key]
    torch = _torch()
    case = wc.BY_NAME[name]
    pb = _pb(case.A)
    pl = hp.make_planner(pb, _pcfg(pb, variant, case.N, case.H, case.k, thr=thr, tau=case.tau if weighted else None))
    ea, em, _ = _noise(1, case.N, case.H, case.A)
    try:
        assert pl.refit() == (('softmax', float(F(case.tau))) if weighted else ('uniform', 0.0)) and pl.select_mode() == 1
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        pl.plan_rollout(0)
        torch.cuda.synchronize()
        out = dict(actions=_np(pl.actions()), ms0=_np(pl.mu_sigma()), launches=pl.launches_per_iteration())
        pl.scores_global().copy_(torch.from_numpy(case.scores))
        torch.cuda.synchronize()
        pl.plan_select(0)
        torch.cuda.synchronize()
        out['elite'], out['ms1'] = _np(pl.elite_idx()), _np(pl.mu_sigma())
        if weighted:
            out['ess'] = pl.refit_stats(0, 1)[0]
        if again:                                                  # a second iteration on the (possibly stopped) handle
            pl.plan_rollout(0)
            pl.plan_select(0)
            torch.cuda.synchronize()
            out['ms2'], out['elite2'] = _np(pl.mu_sigma()), _np(pl.elite_idx())
        out['action'], out['score'], out['iters'] = pl.plan_end(eps_out=np.zeros(case.A, F))
    finally:
        pl.close()
    _RUNS[key] = out
    return out


def _hold(r, case):
    """mu / sigma / ESS of a weighted select against the float64 restatement on the device's own actions and elite set."""
    mu64, sg64, ess64, _, _ = wc.refit64(case.scores, np.sort(r['elite']), r['actions'], r['ms0'][0], r['ms0'][1], SMOOTHING, case.tau)
    err_mu = np.abs(r['ms1'][0] - mu64) / (wc.MU_ATOL + wc.MU_RTOL * np.abs(mu64))
    err_sg = np.abs(r['ms1'][1] - sg64) / (wc.SG_ATOL + wc.SG_RTOL * np.abs(sg64))
    print('%s: mu %.3f, sigma %.3f of the bar; ESS %.6g (float64 %.6g)' % (case.name, err_mu.max(), err_sg.max(), r['ess'], ess64))
    np.testing.assert_allclose(r['ms1'][0], mu64, rtol=wc.MU_RTOL, atol=wc.MU_ATOL)
    np.testing.assert_allclose(r['ms1'][1], sg64, rtol=wc.SG_RTOL, atol=wc.SG_ATOL)
    assert abs(float(r['ess']) - ess64) <= 1e-5 * ess64 and 1.0 <= r['ess'] <= case.k * (1 + 1e-6)
    return float(err_mu.max()), float(err_sg.max())


# ------------------------------------------------------------------------------------------------- 1: op cases
@pytest.mark.parametrize('variant', VARIANTS)
@pytest.mark.parametrize('case', wc.CASES, ids=lambda c: c.name)
def test_weighted_select_op(case, variant):
    w, u = _select_once(case.name, variant, True), _select_once(case.name, variant, False)
    assert w['launches'] == u['launches'] + 1
    # everything the select owns is the uniform handle's, bit for bit, on the same scores
    np.testing.assert_array_equal(w['actions'].view(U), u['actions'].view(U))
    np.testing.assert_array_equal(w['ms0'].view(U), u['ms0'].view(U))
    np.testing.assert_array_equal(w['elite'], u['elite'])
    np.testing.assert_array_equal(np.sort(w['elite']), wc.reference_top_k(case.scores, case.k))
    np.testing.assert_array_equal(w['action'].view(U), u['action'].view(U))
    assert F(w['score']).view(U) == F(u['score']).view(U) and w['iters'] == u['iters'] == 1
    _hold(w, case)
    if case.tau < 1e29 and case.k > 1 and not (np.isneginf(case.scores).all() or case.name == 'budget_all_infeasible'):
        assert not np.array_equal(w['ms1'], u['ms1'])              # (the weights are live)


def test_variants_are_bit_identical_on_the_same_scores():
    """The refit kernel is the same behind the plain and the CROWDED select; the rollouts of the three variants share their actions."""
    for name in ('tau_small', 'safe_crowd', 'wide_k5'):
        c, s, k = (_select_once(name, v, True) for v in VARIANTS)
        for other in (s, k):
            np.testing.assert_array_equal(c['actions'].view(U), other['actions'].view(U))
            np.testing.assert_array_equal(c['ms1'].view(U), other['ms1'].view(U))
            assert F(c['ess']).view(U) == F(other['ess']).view(U)


# ------------------------------------------------------------------------------------------------- 2: exact cases
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_dominant_score_is_exact(variant):
    case = wc.BY_NAME['dominant']
    r = _select_once('dominant', variant, True)
    a = r['actions'][wc.DOMINANT_AT]
    s, oms = F(SMOOTHING), F(1.0 - SMOOTHING)
    np.testing.assert_array_equal(r['ms1'][0].view(U), (s * r['ms0'][0] + oms * a).astype(F).view(U))       # mean == that elite's actions
    np.testing.assert_array_equal(r['ms1'][1].view(U), (s * r['ms0'][1]).astype(F).view(U))                   # sd == 0
    assert r['ess'] == 1.0 and r['score'] == case.scores[wc.DOMINANT_AT]


# ------------------------------------------------------------------------------------------------- 3: early stop
def test_early_stop_is_decided_by_the_weighted_sigma():
    """A threshold between the weighted and the uniform mean sigma of a case: the weighted handle stops after iteration 1 and further
    stepwise calls change nothing; the uniform handle goes on."""
    name = 'tau_small'
    w0, u0 = _select_once(name, 'cem', True), _select_once(name, 'cem', False)
    sw, su = wc.stops(w0['ms1'][1], 0.0)[1], wc.stops(u0['ms1'][1], 0.0)[1]
    assert sw < su                                                 # a few elites carry the weight: the weighted sigma is the smaller
    thr = float((float(sw) + float(su)) / 2)
    assert wc.stops(w0['ms1'][1], thr)[0] and not wc.stops(u0['ms1'][1], thr)[0]
    w, u = _select_once(name, 'cem', True, thr=thr, again=True), _select_once(name, 'cem', False, thr=thr, again=True)
    np.testing.assert_array_equal(w['ms1'].view(U), w0['ms1'].view(U))
    assert w['iters'] == 1 and u['iters'] == 2
    np.testing.assert_array_equal(w['ms2'].view(U), w['ms1'].view(U))              # stopped: the second rollout / select left at once
    np.testing.assert_array_equal(w['elite2'], w['elite'])
    assert not np.array_equal(u['ms2'], u['ms1'])


# ------------------------------------------------------------------------------------------------- 4: whole plans
N_PLAN, K_PLAN, H_PLAN, I_PLAN, TAU_PLAN = 130, 17, 3, 3, 0.5


def _plan_cfg(variant='cem', tau=TAU_PLAN, use_graph=False, **kw):
    return _pcfg(_pb(), variant, N_PLAN, H_PLAN, K_PLAN, I=I_PLAN, tau=tau, use_graph=use_graph, **kw)


@pytest.mark.parametrize('variant', VARIANTS)
def test_whole_plans_stepwise_eager_and_graph(variant):
    torch = _torch()
    pb = _pb()
    pl = hp.make_planner(pb, _plan_cfg(variant))
    pl.plan_begin(pb['state'], seed=5, call=9)
    ess = []
    for it in range(I_PLAN):
        pl.plan_rollout(it)
        torch.cuda.synchronize()
        scores, actions, ms0 = _np(pl.scores_global()), _np(pl.actions()), _np(pl.mu_sigma())
        pl.plan_select(it)
        torch.cuda.synchronize()
        ms1, elite = _np(pl.mu_sigma()), np.sort(_np(pl.elite_idx()))
        np.testing.assert_array_equal(elite, wc.reference_top_k(scores, K_PLAN))
        mu64, sg64, ess64, _, _ = wc.refit64(scores, elite, actions, ms0[0], ms0[1], SMOOTHING, TAU_PLAN)
        np.testing.assert_allclose(ms1[0], mu64, rtol=wc.MU_RTOL, atol=wc.MU_ATOL)
        np.testing.assert_allclose(ms1[1], sg64, rtol=wc.SG_RTOL, atol=wc.SG_ATOL)
        ess.append(pl.refit_stats(0, it + 1)[it])                  # (allowed inside a stepwise plan)
        assert abs(float(ess[-1]) - ess64) <= 1e-5 * ess64
    step = pl.plan_end()
    ms_step = _np(pl.mu_sigma())
    assert step[2] == I_PLAN
    # the same plan through plan(): eager, then twice as a captured graph
    for use_graph in (False, True):
        whole = hp.make_planner(pb, _plan_cfg(variant, use_graph=use_graph))
        for rep in range(2):
            a, s, i = whole.plan(pb['state'], seed=5, call=9)
            assert whole.graph_status() == ('graph' if use_graph else 'eager')
            np.testing.assert_array_equal(a.view(U), step[0].view(U))
            assert F(s).view(U) == F(step[1]).view(U) and i == step[2]
            np.testing.assert_array_equal(_np(whole.mu_sigma()).view(U), ms_step.view(U))
            np.testing.assert_array_equal(whole.refit_stats(0).view(U), np.array(ess, F).view(U))
        assert whole.launches_per_iteration() == pl.launches_per_iteration()
        whole.close()
    pl.close()


# ------------------------------------------------------------------------------------------------- 5: batch
def test_batch_rows_are_their_single_plans():
    torch = _torch()
    from ethz_safe_learning_amd import BatchCemPlanner
    pb = _pb()
    rng = np.random.default_rng(3)
    states = (pb['state'][None] + rng.normal(0, 0.05, (3, pb['state'].shape[0]))).astype(F)
    calls = np.array([4, 5, 6], np.uint64)
    HA2 = 2 * H_PLAN * 2
    rows = {}
    for tau in (TAU_PLAN, None):
        bp = BatchCemPlanner(_plan_cfg('safe', tau=tau, use_graph=True), 4)
        bp.set_weights(pb['weights']); bp.set_normaliser(pb['inputs_min'], pb['inputs_max'])
        acts, scores, iters = bp.plan_batch(states, seed=5, calls=calls)
        rows[tau] = _np(bp._view(bp.layout.mu_sigma, 4 * HA2, torch.float32)).reshape(4, 2, H_PLAN, 2)
        if tau is not None:
            assert bp.graph_status() == 'graph'
            for b in range(3):
                one = hp.make_planner(pb, _plan_cfg('safe', use_graph=True))
                a, s, i = one.plan(states[b], seed=5, call=int(calls[b]))
                np.testing.assert_array_equal(acts[b].view(U), a.view(U))
                assert F(scores[b]).view(U) == F(s).view(U) and iters[b] == i
                np.testing.assert_array_equal(rows[tau][b].view(U), _np(one.mu_sigma()).view(U))
                np.testing.assert_array_equal(bp.refit_stats(b, int(i)).view(U), one.refit_stats(0, int(i)).view(U))
                one.close()
        bp.close()
    # the row that sat the plan out: what the first kernel left there, whatever the refit
    np.testing.assert_array_equal(rows[TAU_PLAN][3].view(U), rows[None][3].view(U))
    assert not np.array_equal(rows[TAU_PLAN][0], rows[None][0])


# ------------------------------------------------------------------------------------------------- 6: warm start
def test_the_carry_is_the_weighted_distribution():
    _torch()
    pb = _pb()
    pl = hp.make_planner(pb, _plan_cfg('cem', use_graph=True))
    pl.set_warm_start(shift=1)
    pl.set_init_mode('shift')
    pl.plan(pb['state'], seed=5, call=9)
    ms = _np(pl.mu_sigma())
    mu, sg, valid = pl.carry(0)
    assert valid
    np.testing.assert_array_equal(mu.view(U), ms[0].view(U))
    np.testing.assert_array_equal(sg.view(U), ms[1].view(U))
    cold = hp.make_planner(pb, _plan_cfg('cem', use_graph=True))
    cold.plan(pb['state'], seed=5, call=9)
    np.testing.assert_array_equal(_np(cold.mu_sigma()).view(U), ms.view(U))         # (the first plan of a warm handle is a cold one)
    a2 = pl.plan(pb['state'], seed=5, call=10)                     # ... and the next one starts from the shifted weighted carry
    c2 = cold.plan(pb['state'], seed=5, call=10)
    assert not np.array_equal(a2[0], c2[0])
    mu2, sg2, valid2 = pl.carry(0)
    assert valid2
    np.testing.assert_array_equal(mu2.view(U), _np(pl.mu_sigma())[0].view(U))
    pl.close(); cold.close()


# ------------------------------------------------------------------------------------------------- 7: round trip
def test_back_on_uniform_the_handle_is_a_fresh_one():
    torch = _torch()
    pb = _pb()
    pl = hp.make_planner(pb, _plan_cfg('cem', tau=None, use_graph=True))
    fresh = hp.make_planner(pb, _plan_cfg('cem', tau=None, use_graph=True))
    base = fresh.launches_per_iteration()
    pl.set_refit('softmax', 0.5)
    assert pl.refit() == ('softmax', 0.5) and pl.launches_per_iteration() == base + 1
    r1 = pl.plan(pb['state'], seed=5, call=9)
    assert pl.graph_status() == 'graph'
    ms1 = _np(pl.mu_sigma())
    pl.set_refit('softmax', 0.5)                                   # the same setting: nothing is dropped
    assert pl.graph_status() == 'graph'
    pl.set_refit('softmax', 0.25)                                  # the temperature alone: captured anew, another result
    assert pl.graph_status() == 'eager' and pl.refit() == ('softmax', 0.25)
    pl.plan(pb['state'], seed=5, call=9)
    assert pl.graph_status() == 'graph' and not np.array_equal(_np(pl.mu_sigma()), ms1)
    pl.set_refit('uniform')
    assert pl.refit() == ('uniform', 0.0) and pl.graph_status() == 'eager' and pl.launches_per_iteration() == base
    a, s, i = pl.plan(pb['state'], seed=5, call=9)
    fa, fs, fi = fresh.plan(pb['state'], seed=5, call=9)
    np.testing.assert_array_equal(a.view(U), fa.view(U))
    assert F(s).view(U) == F(fs).view(U) and i == fi and pl.graph_status() == fresh.graph_status() == 'graph'
    for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'returns'):
        assert torch.equal(getattr(pl, view)(), getattr(fresh, view)()), view
    assert not np.array_equal(r1[0], a) or r1[1] != s or not np.array_equal(ms1, _np(pl.mu_sigma()))
    pl.close(); fresh.close()


# ------------------------------------------------------------------------------------------------- 8: refusals
def _status(fn, *a, **kw):
    from ethz_safe_learning_amd._capi import CemError
    with pytest.raises(CemError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals():
    _torch()
    pb = _pb()
    # world_size > 1, select_mode 2, a population the automatic choice gives to a multi-workgroup select
    for kw in (dict(world_size=2, rank=0), dict(select_mode=2), dict(N=24000, k=100)):
        shape = dict(dict(N=N_PLAN, k=K_PLAN), **{k: kw[k] for k in ('N', 'k') if k in kw})
        extra = {k: v for k, v in kw.items() if k not in ('N', 'k')}
        pl = hp.make_planner(pb, _pcfg(pb, 'cem', shape['N'], H_PLAN, shape['k'], I=2, **extra))
        assert _status(pl.set_refit, 'softmax', 0.5) == UNSUPPORTED
        assert pl.refit() == ('uniform', 0.0)
        pl.set_refit('uniform')                                     # the default is always accepted
        if not extra.get('world_size'):
            a, s, i = pl.plan(pb['state'], seed=1, call=0)          # ... and the handle still plans
            assert np.isfinite(a).all() and i == 2
        pl.close()
        with pytest.raises(Exception):
            hp.make_planner(pb, _pcfg(pb, 'cem', shape['N'], H_PLAN, shape['k'], I=2, tau=0.5, **extra))
    pl = hp.make_planner(pb, _pcfg(pb, 'safe', N_PLAN, H_PLAN, K_PLAN, I=2))
    for tau in (0.0, -1.0, float('nan'), float('inf'), -0.0):
        assert _status(pl.set_refit, 'softmax', tau) == INVALID_ARG
    assert pl.lib.cem_planner_set_refit(pl.h, 2, 1.0) == INVALID_ARG
    assert _status(pl.refit_stats, 0, 1) == STATE                  # no weighted select has run
    pl.set_refit('softmax', 0.5)
    assert _status(pl.refit_stats, 1, 1) == INVALID_ARG and _status(pl.refit_stats, 0, 3) == INVALID_ARG
    assert pl.lib.cem_planner_refit_stats(pl.h, 0, None, 1) == INVALID_ARG
    # inside a stepwise plan
    pl.plan_begin(pb['state'], seed=1, call=0)
    assert _status(pl.set_refit, 'uniform') == STATE
    assert _status(pl.set_refit, 'softmax', 0.25) == STATE
    for it in range(2):
        pl.plan_rollout(it); pl.plan_select(it)
    a, s, i = pl.plan_end()
    assert pl.refit() == ('softmax', 0.5) and i == 2 and np.isfinite(a).all()
    assert (pl.refit_stats(0, 2) >= 1.0).all()
    pl.close()


# ------------------------------------------------------------------------------------------------- 9: the policies
def _policy(name, seed=3, **extra):
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    env, model, pol = make_agent_parts(name, seed=seed)
    trained_like(model, np.random.default_rng(0))
    if extra:
        pol = (SafeCemMpc if name == 'safe_cem_mpc' else CemMpc)(model=model, environment=env, **dict(POLICIES_YAML[name], **extra))
    return env, pol


def _states(n):
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    return np.stack([PointGoalEnv(seed=s).reset() for s in range(n)]).astype(F)


@pytest.mark.parametrize('name,extra', [('cem_mpc', {}), ('safe_cem_mpc', dict(cost_budget=25.0))], ids=['cem', 'safe_budget'])
def test_policies_plan_with_an_elite_temperature(name, extra):
    _torch()
    states = _states(3)
    env, pol = _policy(name, elite_temperature=0.5, **extra)
    cfg = pol.planner_config()
    assert (cfg.refit, cfg.refit_temperature) == ('softmax', 0.5)
    pol.build_batch(3)._call = 50
    acts = pol.generate_actions(states)
    assert acts.shape == (3, 2) and (acts >= env.action_space.low - 0.1).all() and (acts <= env.action_space.high + 0.1).all()
    assert len(pol.last_ess) == 3
    ess_rows, iters_rows = list(pol.last_ess), np.array(pol.last_iterations)   # (generate_action below overwrites both)
    for b in range(3):
        ess = ess_rows[b]
        assert ess.shape == (int(iters_rows[b]),) and (ess >= 1.0).all() and (ess <= pol.elite * (1 + 1e-6)).all()
        pol.build(); pol._planner._call = 50 + b
        a = pol.generate_action(states[b])
        assert pol._planner.refit() == ('softmax', 0.5) and pol._planner.graph_status() == 'graph'
        np.testing.assert_array_equal(a.view(U), acts[b].view(U))                  # a row of the batch is its single plan
        np.testing.assert_array_equal(pol.last_ess.view(U), ess.view(U))
    if name == 'safe_cem_mpc':
        assert pol.cost_planner_config().refit == 'uniform'        # optimize_for_safety and the recovery plans keep the uniform refit
        pol.optimize_for_safety(states[0], call=1)
        assert pol._cost_planner.refit() == ('uniform', 0.0)


def test_policy_without_a_temperature_is_the_parent_policy():
    _torch()
    from ethz_safe_learning_amd.planner import config_key, planner_cache_info
    st = _states(1)[0]
    _, plain = _policy('cem_mpc')
    plain.build(); plain._planner._call = 50
    a_plain = plain.generate_action(st)
    n_handles = planner_cache_info()['size']
    _, none = _policy('cem_mpc', elite_temperature=None)
    none.build(); none._planner._call = 50
    assert none._planner is plain._planner and planner_cache_info()['size'] == n_handles
    np.testing.assert_array_equal(none.generate_action(st).view(U), a_plain.view(U))
    assert none.last_score == plain.last_score and none._planner.refit() == ('uniform', 0.0) and none.last_ess is None
    assert config_key(none.planner_config()) == config_key(plain.planner_config())
    with pytest.raises(ValueError):
        _policy('cem_mpc', elite_temperature=0.0)
