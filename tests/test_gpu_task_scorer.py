"""The task scorer (cem_planner_set_task) on the device.

The kernel has an exact reference that costs nothing: planner.task_objective restates it bit for bit, and everything it reads — the
trajectories the MODE 1 rollout wrote, the sample — can be copied out of the handle after every launch.  So (1) the kernel alone is held
to the mirror on random and crafted tensors, (2) the trajectories a plan scores are held to cem_unfold_sequences, (3) a plan's scores
to the existing score kernels' restatements applied to the mirror, and the rest — the plan forms, the other options, off is off, the
refusals, a closed loop on a non-lidar environment — hangs off that."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner, _capi
from ethz_safe_learning_amd.planner import QuadraticTask, task_objective
from tests import constrained_cases as cc
from tests import cost_cases
from tests import helpers as hp
from tests import risk_cases as rk
from tests import task_cases as tc

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
N, P, E, H, K = 50, 3, 3, 7, 5
SEED = 5


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 64
RET_GUARD, COST_GUARD = 0x7fa5a5a5, 0xa5


def _run_kernel(pl, tr, act, misalign=False):
    """cem_task_score on host arrays through guarded device buffers -> (ret [rows], cost bytes [H, rows] as the buffer holds them)."""
    t = _torch()
    rows, H1, _ = tr.shape
    Hh = H1 - 1
    flat = t.zeros(tr.size + 4, dtype=t.float32, device=pl.device)
    off = 1 if misalign else 0                                                 # one float off a 16-byte boundary: the element path
    flat[off:off + tr.size] = t.from_numpy(tr.reshape(-1)).to(pl.device)
    traj = flat[off:off + tr.size]
    a = t.from_numpy(act).to(pl.device).contiguous()
    ret = t.from_numpy(np.full(rows + GUARD, RET_GUARD, np.uint32).view(np.int32)).to(pl.device)
    costs = t.full((Hh * rows + GUARD,), COST_GUARD, dtype=t.uint8, device=pl.device)
    t.cuda.synchronize()
    _capi.check(pl.lib.cem_task_score(pl.h, C.c_void_p(traj.data_ptr()), C.c_void_p(a.data_ptr()), rows, Hh, C.c_void_p(ret.data_ptr()),
                                      C.c_void_p(costs.data_ptr())), 'cem_task_score')
    r, c = _np(ret).view(np.uint32), _np(costs)
    assert (r[rows:] == RET_GUARD).all() and (c[Hh * rows:] == COST_GUARD).all(), 'a guard word behind an output was written'
    return r[:rows].view(F), c[:Hh * rows].reshape(Hh, rows)


@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('shape', tc.SHAPES, ids=lambda s: 'O%d_A%d_H%d_rows%d_P%d' % s)
def test_kernel_equals_the_mirror(shape, variant):
    """Returns and cost bytes bit for bit, random rows and the crafted ones (on a bound, one ulp outside, near at exactly R2, the goal
    at t = 0 / at the last step / never, a NaN feature), with the reward clip active on about half of the steps; guard words behind
    both outputs stay; a 'cem' handle writes no cost byte at all.  The 16-byte shapes run a second time one float off alignment."""
    _torch()
    O, A, Hh, rows, Pp = shape
    task = tc.task_for(O, A, 0, True)
    pl = CemPlanner(dataclasses.replace(tc.kernel_handle_config(O, A, Pp, variant), task=task))
    try:
        tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
        names = tc.craft(tr, task)
        want_ret, want_costs, first = task_objective(tr, act, task, variant, return_done=True)
        if rows > 8 and Hh >= 3:
            assert {'on_bounds', 'ulp_below_lo', 'near_exactly', 'goal_at_0', 'goal_at_last_step', 'goal_never', 'nan_feature'} <= set(names)
            assert (first < Hh).any() and (first == Hh).any()
        for misalign in ([False, True] if O % 4 == 0 else [False]):
            ret, costs = _run_kernel(pl, tr, act, misalign)
            _bits(ret, want_ret, 'returns (misalign %s)' % misalign)
            if variant == 'cem':
                assert (costs == COST_GUARD).all()
            else:
                _bits(costs, want_costs, 'cost bytes (misalign %s)' % misalign)
                assert rows < 9 or (want_costs.any() and not want_costs.all())
        # the clip off too (returns reach -inf on the NaN row)
        pl.set_task(tc.task_for(O, A, 0, False))
        ret, _ = _run_kernel(pl, tr, act)
        _bits(ret, task_objective(tr, act, tc.task_for(O, A, 0, False), variant)[0], 'returns without a clip')
    finally:
        pl.close()


def test_kernel_on_a_cost_handle_masks_nothing():
    _torch()
    O, A, Hh, rows, Pp = tc.SHAPES[1]
    task = tc.task_for(O, A, 1, True)
    pl = CemPlanner(dataclasses.replace(tc.kernel_handle_config(O, A, Pp, 'cost'), task=task))
    try:
        tr, act = tc.random_case(O, A, Hh, rows, Pp, 1)
        tc.craft(tr, task)
        ret, costs = _run_kernel(pl, tr, act)
        want_ret, want_costs = task_objective(tr, act, task, 'cost')
        _bits(ret, want_ret)
        _bits(costs, want_costs)
        assert want_costs.sum() > task_objective(tr, act, task, 'safe')[1].sum()          # (the safe variant's mask removes some)
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# plans: the handles of sections 2 - 5
# ---------------------------------------------------------------------------------------------------------------------------------
HANDLES = {
    'fp32_obs60': dict(obs=60),
    'fp32_obs84': dict(obs=84),
    'units160_wide': dict(obs=60, units=160),
    'bf16x3': dict(obs=60, precision='bf16x3'),
    'bf16': dict(obs=60, precision='bf16'),
}
_PROBLEMS = {}


def _problem(obs=60, units=128):
    key = (obs, units)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = hp.make_problem(obs_dim=obs, act_dim=2, E=E, n_layers=4, seed=77, units=units)
    return _PROBLEMS[key]


def _configs(obs=60, units=128, precision='fp32', variant='cem', I=2, **kw):
    pb = _problem(obs, units)
    _, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=K, I=I, variant=variant, precision=precision, post=0.3, **kw)
    return pb, pcfg


def _run_all(pl, state, seed, call, **noise):
    """One stepwise plan to its end -> (per iteration: trajectories, actions, scores, returns, cost bytes), result."""
    per = []
    pl.plan_begin(state, seed, call, **noise)
    for it in range(pl.cfg.iterations):
        pl.plan_rollout(it)
        per.append(dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                        returns=_np(pl.returns()).reshape(-1), costs=_np(pl.costs()).reshape(-1)))
        pl.plan_select(it)
    return per, pl.plan_end()


def _calibrated_task(pl, pb, clip=False):
    """A task whose thresholds are taken from the handle's own first rollout, so that both outcomes of every comparison occur on what
    it predicts: the goal on features 0 and 1, a little off the start state (which would be near at t = 0 on every row), with R2 the
    median over the rows of the closest a row gets to it after t = 0; a box between the 10 % and 90 % quantiles of features 2 .. 9.
    (Thresholds of the TEST's task, not bars: every check below is bit for bit against the mirror on the device's own trajectories.)"""
    O = pb['state'].shape[0]
    pl.set_task(QuadraticTask(q=1.0, g=pb['state']))
    per, _ = _run_all(pl, pb['state'], SEED, 900)
    tr = per[0]['traj'].astype(np.float64)
    g = pb['state'].astype(np.float64).copy()
    sd = tr[:, H // 2, :2].std(axis=0)
    for mult in (1.0, 2.0, 4.0, 0.5):
        g[:2] = pb['state'][:2] + mult * sd
        nsum = ((tr[:, :H, :2] - g[:2]) ** 2).sum(axis=2)                  # [rows, H]: near(s_t) is asked for t < H
        r2 = float(np.median(nsum[:, 1:].min(axis=1)))
        if r2 < 0.98 * nsum[0, 0]:
            break
    radius = float(np.sqrt(r2))
    g = g.astype(F)
    lo, hi, m = np.full(O, -np.inf, F), np.full(O, np.inf, F), np.zeros(O, F)
    lo[2:10] = np.quantile(tr[:, 1:, 2:10], 0.1, axis=(0, 1))
    hi[2:10] = np.quantile(tr[:, 1:, 2:10], 0.9, axis=(0, 1))
    m[:2] = 1.0
    rng = np.random.default_rng(3)
    task = QuadraticTask(q=rng.uniform(0.0, 1.0, O).astype(F), g=g, c=rng.normal(0, 0.01, O).astype(F), goal_mask=m, lo=lo, hi=hi,
                         rho=[0.1, 0.2], goal_radius=radius, reward_goal=0.05, reward_clip=0.0)
    if clip:
        ret, _ = task_objective(per[0]['traj'], per[0]['actions'], task, 'cem')
        task = dataclasses.replace(task, reward_clip=float(np.median(np.abs(ret)) / H))
    pl.set_task(task)
    return task


def _planner(name='fp32_obs60', variant='cem', calibrate=True, **kw):
    _torch()
    spec = dict(HANDLES[name])
    pb, pcfg = _configs(variant=variant, **spec, **kw)
    pl = hp.make_planner(pb, pcfg)
    task = _calibrated_task(pl, pb) if calibrate else None
    return pb, pcfg, pl, task


def _restated_scores(variant, ret, costs, pcfg, n):
    """The existing score kernels' NumPy statements (tests/constrained_cases.py, risk_cases.py, cost_cases.py) on returns [P n] and
    cost bytes [H, P n]."""
    r = ret.reshape(P, n)
    if variant == 'cem':
        return cc.mean_returns(r)
    cb = costs.reshape(H, P, n)
    if variant == 'cost':
        return cost_cases.scores_from_bytes(cb, P, n)
    unsafe = rk.unsafe_flags(cb, P, pcfg.posterior_mean_threashold)
    return cc.mean_returns(r) - np.where(unsafe, F(1.0), F(0.0)) * F(100.0)


def _check_iteration(rec, task, variant, pcfg, n=N, what=''):
    """One iteration's returns, cost bytes and scores against the mirror on the trajectories and the sample the device itself held."""
    traj, act = rec['traj'][:P * n], rec['actions'][:n]
    ret, costs = task_objective(traj, act, task, variant)
    _bits(rec['returns'][:P * n], ret, '%s: returns' % what)
    if variant != 'cem':
        _bits(rec['costs'][:H * P * n].reshape(H, P * n), costs, '%s: cost bytes' % what)
    _bits(rec['scores'][:n], _restated_scores(variant, ret, costs, pcfg, n), '%s: scores' % what)
    return ret, costs


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the trajectories a plan scores are cem_unfold_sequences' on the same actions and model noise
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(HANDLES))
def test_trajectories_equal_unfold_sequences(name):
    t = _torch()
    pb, pcfg, pl, _ = _planner(name, calibrate=False)
    try:
        pl.set_task(QuadraticTask(q=1.0, g=pb['state']))
        assert pl.rollout_path() == 'generic'
        ea, em, _ = pl.fill_noise(SEED, 3)
        per, _ = _run_all(pl, pb['state'], SEED, 3, eps_act=ea, eps_model=em)
        O = pcfg.obs_dim
        B = P * N
        rc_, tiles = pl.tiles()
        row_of, act_of = np.full(B, -1), np.full(B, -1)            # by GLOBAL row id (the Philox / eps_model row): the local row and the candidate
        for row_base, cnt, member, act_base, noise_base, s0_base in tiles:
            assert s0_base == -1
            g = noise_base + np.arange(cnt)
            assert ((g // (B // E)) == member).all()                # the member unfold_sequences gives the same global row
            row_of[g], act_of[g] = row_base + np.arange(cnt), act_base + np.arange(cnt)
        assert sorted(row_of) == list(range(B)) and (act_of == row_of % N).all()      # row r belongs to candidate r mod N
        for it in range(pcfg.iterations):
            acts = t.from_numpy(per[it]['actions'][act_of]).to(pl.device)
            s0 = t.from_numpy(np.tile(pb['state'].astype(F), (B, 1))).to(pl.device)
            want = _np(pl.unfold_sequences(s0, acts, eps_model=em[it]))
            assert per[it]['traj'].shape == (B, H + 1, O)
            _bits(per[it]['traj'][row_of], want, '%s iteration %d' % (name, it))
            assert not np.array_equal(per[it]['traj'][:, 0], per[it]['traj'][:, H])
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. a plan's scores; graph, eager and stepwise plans
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['cem', 'safe', 'cost'])
def test_scores_of_two_iterations_and_the_three_plan_forms(variant):
    pb, pcfg, pl, task = _planner(variant=variant)
    others = []
    try:
        per, (a, s, iters) = _run_all(pl, pb['state'], SEED, 0)
        seen_done = seen_cost = False
        for it in range(2):
            ret, costs = _check_iteration(per[it], task, variant, pcfg, what='%s iteration %d' % (variant, it))
            first = task_objective(per[it]['traj'], per[it]['actions'], task, variant, return_done=True)[2]
            seen_done |= bool((first < H).any() and (first == H).any())
            seen_cost |= costs is not None and bool(costs.any() and not costs.all())
        assert seen_done or variant == 'cost'                      # the calibrated thresholds fall on both sides
        assert seen_cost or variant == 'cem'
        assert not np.array_equal(per[0]['scores'], per[1]['scores'])
        # eager and graph plans on handles of their own, Philox noise: the same action, score and iteration count
        for use_graph in (False, True):
            _, cfg2 = _configs(variant=variant, use_graph=use_graph)
            p2 = hp.make_planner(pb, dataclasses.replace(cfg2, task=task))
            others.append(p2)
            for _ in range(2):                                     # (the second graph plan replays the captured one)
                a2, s2, i2 = p2.plan(pb['state'], seed=SEED, call=0)
                _bits(a2, a, 'action, use_graph %s' % use_graph)
                assert F(s2).view(U) == F(s).view(U) and i2 == iters
            assert p2.graph_status() == ('graph' if use_graph else 'eager')
            assert p2.rollout_path() == 'generic' and p2.iteration_plan(0)['rollout_path'] == 'generic'
    finally:
        for p in [pl] + others:
            p.close()


def test_an_active_clip_in_a_plan():
    pb, pcfg, pl, _ = _planner(calibrate=False)
    try:
        task = _calibrated_task(pl, pb, clip=True)
        per, _ = _run_all(pl, pb['state'], SEED, 1)
        _check_iteration(per[0], task, 'cem', pcfg, what='clip')
    finally:
        pl.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. one small case each with the other options
# ---------------------------------------------------------------------------------------------------------------------------------
def test_with_risk_level():
    pb, pcfg, pl, task = _planner()
    try:
        pl.set_particle_objective('lower_tail', 2)
        per, _ = _run_all(pl, pb['state'], SEED, 0)
        ret, _ = task_objective(per[0]['traj'], per[0]['actions'], task, 'cem')
        _bits(per[0]['scores'], rk.scores(ret.reshape(P, N), 2), 'lower-tail scores')
    finally:
        pl.close()


def test_with_cost_budget():
    pb, pcfg, pl, task = _planner(variant='safe')
    try:
        pl.set_constraint('budget', 0)
        pl.set_cost_budget(1.0)
        per, _ = _run_all(pl, pb['state'], SEED, 0)
        ret, costs = task_objective(per[0]['traj'], per[0]['actions'], task, 'safe')
        want = cc.scores(ret.reshape(P, N), costs.reshape(H, P, N), P, N, P, 1.0)
        _bits(per[0]['scores'], want, 'budget scores')
        feas = cc.feasible(costs.reshape(H, P, N), P, N, P, 1.0)
        assert feas.any() and not feas.all()
    finally:
        pl.close()


def test_with_plan_readout():
    pb, pcfg, pl, task = _planner(I=1)
    try:
        pl.set_plan_readout(True)
        a, s, _ = pl.plan(pb['state'], seed=SEED, call=0)
        ro = pl.plan_readout()
        ret, _ = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'cem')
        assert ro.iteration == 0 and 0 <= ro.candidate < N
        _bits(ro.particle_returns, ret.reshape(P, N)[:, ro.candidate], 'particle returns of the winner')
        _bits(ro.sequence[0], a)
        assert F(ro.score).view(U) == F(cc.mean_returns(ret.reshape(P, N))[ro.candidate]).view(U) == F(s).view(U)
    finally:
        pl.close()


def test_with_population_decay():
    pb, pcfg, pl, task = _planner()
    n1 = 35
    try:
        pl.set_population_schedule([N, n1])
        assert pl.iteration_plan(1)['n_samples'] == n1 and pl.iteration_plan(1)['rollout_path'] == 'generic'
        pl.plan_begin(pb['state'], SEED, 0)
        pl.plan_rollout(0)
        rec0 = dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                    returns=_np(pl.returns()).reshape(-1), costs=None)
        _check_iteration(rec0, task, 'cem', pcfg, what='iteration 0')
        pl.plan_select(0)
        # rows beyond n[1]: poisoned before the narrower iteration, untouched and unread by it
        pl.returns().reshape(-1)[P * n1:] = float('nan')
        pl.scores_local()[n1:] = float('nan')
        pl.plan_rollout(1)
        rec1 = dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                    returns=_np(pl.returns()).reshape(-1), costs=None)
        _check_iteration(rec1, task, 'cem', pcfg, n=n1, what='iteration 1')
        assert np.isnan(rec1['returns'][P * n1:]).all() and np.isnan(rec1['scores'][n1:]).all()
        _bits(rec1['traj'][P * n1:], rec0['traj'][P * n1:], 'trajectory rows beyond the narrower population')
        pl.plan_select(1)
        _, score, iters = pl.plan_end()
        assert np.isfinite(score) and iters == 2
    finally:
        pl.close()


def test_timed_plan_is_the_same_plan_and_times_the_kernel_with_the_reduce():
    pb, pcfg, pl, task = _planner()
    try:
        a, s, i = pl.plan(pb['state'], seed=SEED, call=0)
        assert pl.last_timing()['reduce_ms'] == 0.0
        pl.set_timing(True)
        a2, s2, i2 = pl.plan(pb['state'], seed=SEED, call=0)
        pl.synchronize()
        _bits(a2, a)
        assert F(s2).view(U) == F(s).view(U) and i2 == i
        tm = pl.last_timing()
        assert tm['reduce_ms'] > 0.0 and tm['rollout_launches'] == i and tm['sampler_ms'] > 0.0
    finally:
        pl.close()


def test_with_warm_start():
    pb, pcfg, pl, task = _planner()
    _, cfg_g = _configs(use_graph=True)
    pg = hp.make_planner(pb, dataclasses.replace(cfg_g, task=task))
    try:
        for p in (pl, pg):
            p.set_warm_start(shift=1)
            p.set_init_mode('shift')
            p.reset_carry()                                        # (the calibration plans left one on the first handle)
        for call in range(2):
            a, s, i = pl.plan(pb['state'], seed=SEED, call=call)
            ag, sg, ig = pg.plan(pb['state'], seed=SEED, call=call)
            _bits(ag, a, 'warm plan %d' % call)
            assert F(sg).view(U) == F(s).view(U) and ig == i
            assert pl.carry()[2] and pg.carry()[2]
        _bits(pg.carry()[0], pl.carry()[0])
    finally:
        pl.close(); pg.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. off is off; refusals
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_set_then_clear_is_a_handle_that_never_had_a_task(variant):
    _torch()
    pb, pcfg = _configs(variant=variant, use_graph=True)
    never, cleared = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    try:
        cleared.set_task(tc.task_for(60, 2))
        on_plan = cleared.iteration_plan(0)
        cleared.plan(pb['state'], seed=SEED, call=0)
        assert cleared.rollout_path() == 'generic'
        cleared.set_task(None)
        assert cleared.task is None
        assert cleared.rollout_path() == never.rollout_path()
        assert [cleared.iteration_plan(i) for i in range(2)] == [never.iteration_plan(i) for i in range(2)]
        assert on_plan['launches'] > never.iteration_plan(0)['launches']               # (the task's extra launches were reported)
        for call in range(2):
            a, s, i = never.plan(pb['state'], seed=SEED, call=call)
            a2, s2, i2 = cleared.plan(pb['state'], seed=SEED, call=call)
            _bits(a2, a)
            assert F(s2).view(U) == F(s).view(U) and i2 == i
        assert cleared.graph_status() == never.graph_status() == 'graph' and cleared.graph_nodes() == never.graph_nodes() > 0
        _bits(_np(cleared.result_block())[:36], _np(never.result_block())[:36])          # (action, score, iterations, flags; [36], [37]: the plan counter and its checksum)
        with pytest.raises(_capi.CemError) as e:
            cleared.task_trajectories()
        assert e.value.status == STATE
    finally:
        never.close(); cleared.close()


def test_refusals():
    _torch()
    pb, pcfg = _configs()
    task = tc.task_for(60, 2)
    pl = hp.make_planner(pb, pcfg)
    try:
        before = pl.iteration_plan(0)
        bad = [dataclasses.replace(task, q=np.full(60, np.nan, F)), dataclasses.replace(task, rho=[np.inf, 0.0]),
               dataclasses.replace(task, lo=1.0, hi=0.5), dataclasses.replace(task, goal_radius=-0.1),
               dataclasses.replace(task, lo=np.full(60, np.nan, F)), dataclasses.replace(task, goal_mask=np.full(60, -np.inf, F))]
        for b in bad:
            with pytest.raises(_capi.CemError) as e:
                pl.set_task(b)
            assert e.value.status == INVALID_ARG
        ct = _capi.CemTask(kind=7)
        assert pl.lib.cem_planner_set_task(pl.h, C.byref(ct)) == INVALID_ARG
        assert pl.iteration_plan(0) == before and pl.task is None
        pl.plan_begin(pb['state'], SEED, 0)
        with pytest.raises(_capi.CemError) as e:
            pl.set_task(task)
        assert e.value.status == STATE
        for it in range(pcfg.iterations):
            pl.plan_rollout(it); pl.plan_select(it)
        pl.plan_end()
    finally:
        pl.close()
    bp = BatchCemPlanner(pcfg, 2)
    try:
        with pytest.raises(_capi.CemError) as e:
            bp.set_task(task)
        assert e.value.status == UNSUPPORTED
        bp.set_task(None)
    finally:
        bp.close()
    with pytest.raises(_capi.CemError) as e:
        BatchCemPlanner(dataclasses.replace(pcfg, task=task), 2)
    assert e.value.status == UNSUPPORTED
    _, cfg_w = _configs(world_size=2)
    pw = CemPlanner(cfg_w)
    try:
        with pytest.raises(_capi.CemError) as e:
            pw.set_task(task)
        assert e.value.status == UNSUPPORTED
    finally:
        pw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. it plans a non-lidar environment
# ---------------------------------------------------------------------------------------------------------------------------------
def test_closed_loop_on_a_double_integrator():
    """CemMpc(task=...) drives a double integrator (obs = (pos, vel), one action, the ensemble set by hand to its exact dynamics, model
    noise off) from pos 1 at rest towards the origin: N = 64, H = 10, I = 3, 40 decisions.  The bar comes from a NumPy CEM on the same
    model (task_cases.reference_closed_loop: planner.task_objective and the oracle's select_and_refit), seeds 0 .. 4, measured on the
    CPU: its worst final stage cost q (s - g)^2 is 2.61e-4, its largest |vel| 0.911 — inside the task's box of 1.0, so its worst
    violation is 0.  The policy's final stage cost stays within 2 x 2.61e-4 and its executed trajectory never leaves the box."""
    _torch()
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    c = tc.INTEGRATOR
    box = lambda lo, hi: types.SimpleNamespace(low=np.asarray(lo, F), high=np.asarray(hi, F), shape=(len(lo),))
    obs_space, act_space = box([-10.0, -10.0], [10.0, 10.0]), box([-1.0], [1.0])
    model = TransitionModel('mlp_ensemble', obs_space, act_space, scale_features=False, sampling_propagation=False, ensemble_size=c['E'],
                            mlp_params=dict(n_layers=2, units=tc.UNITS, activation='tf.nn.relu', dropout_rate=0.0))
    model.model.set_weights(tc.integrator_weights(c['E']))
    env = types.SimpleNamespace(action_space=act_space, observation_space=obs_space)
    pol = CemMpc(model=model, environment=env, horizon=c['H'], iterations=c['I'], smoothing=0.0, n_samples=c['N'], n_elite=c['k'],
                 particles=c['P'], stddev_threshold=-1.0, noise_stddev=0.0, seed=SEED, task=tc.INTEGRATOR_TASK)
    s = np.array([1.0, 0.0], F)
    vmax = 0.0
    for step in range(c['steps']):
        a = pol.generate_action(s)
        if step == 0:
            pl = pol._planner
            assert pl.task is tc.INTEGRATOR_TASK and pl.rollout_path() == 'generic'
            # the hand-set model IS the dynamics: the trajectories the plan scored follow integrator_step on the plan's own actions
            traj, acts = _np(pl.task_trajectories()), _np(pl.actions())
            want = np.zeros((c['N'], c['H'] + 1, 2), F)
            want[:, 0] = s
            for t in range(c['H']):
                want[:, t + 1] = tc.integrator_step(want[:, t], acts[:, t, 0])
            np.testing.assert_allclose(traj, np.tile(want, (c['P'], 1, 1)), rtol=0, atol=2e-6)
        s = tc.integrator_step(s, a[0])
        vmax = max(vmax, abs(float(s[1])))
    cost = tc.stage_cost(s)
    print('double integrator: final stage cost %.3g (reference worst %.3g), largest |vel| %.3f' % (cost, tc.REFERENCE_WORST_STAGE_COST, vmax))
    assert cost <= 2 * tc.REFERENCE_WORST_STAGE_COST, cost
    assert vmax <= tc.VEL_BOX, vmax
    with pytest.raises(ValueError, match='batch handle'):
        pol.generate_actions(np.zeros((2, 2), F))
