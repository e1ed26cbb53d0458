"""Zones on a task (cem_planner_set_task_zones) on the device.

The kernel has an exact reference that costs nothing: planner.task_objective / tracking_objective restate cem_task_zones_kernel bit for
bit (tests/test_zones_cpu.py holds that mirror to a float64 statement of the contract).  So (1) the kernel alone is held to the mirror on
random and crafted tensors over both base kinds, (2) a plan's returns, cost bytes and scores to the mirror on the trajectories the handle
itself kept, in every plan form, (3) zones that do nothing and zones that were cleared are shown to leave the base task's bits, and the
rest — the other options, the refusals, a closed loop round a disc — hangs off that."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner, StateZones, _capi
from ethz_safe_learning_amd.planner import QuadraticTask, TrackingTask, task_objective, tracking_objective, zone_terms
from tests import constrained_cases as cc
from tests import cost_cases
from tests import helpers as hp
from tests import risk_cases as rk
from tests import task_cases as tc
from tests import tracking_cases as tk
from tests import zone_cases as zc

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
N, P, E, H, K = 64, 2, 2, 10, 8
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


def _objective(task, tr, act, variant, k0=0, prev=None, **kw):
    if isinstance(task, TrackingTask):
        return tracking_objective(tr, act, task, variant, k0=k0, prev_action=prev, **kw)
    return task_objective(tr, act, task, variant, **kw)


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


def _kernel_cases(O, A, Hh, rows, Pp, kind):
    """(name, task, traj, actions, k0, prev): random states under random zones over the base task's own crafted rows; the crafted zone
    rows; sixteen active zones (O >= 57)."""
    if kind == 'quadratic':
        base, k0, prev = tc.task_for(O, A, 0, True), 0, None
    else:
        base, k0, prev = tk.tracking_task_for(O, A, Hh + 1, 0, True), 3, tk.prev_action_for(A)
    tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
    if kind == 'quadratic':
        tc.craft(tr, base)
    else:
        tk.craft(tr, act, base, k0, prev)
    yield 'random', zc.with_zones(base, zc.random_zones(O, 0)), tr, act, k0, prev
    if O >= 57:
        cbase, g, ck0, cprev = zc.crafted_base(O, A, kind, Hh)
        task, ctr, cact, _ = zc.crafted_case(cbase, O, A, Hh, Pp, g)
        yield 'crafted', task, ctr, cact, ck0, cprev
        yield 'sixteen', zc.with_zones(base, zc.sixteen_zones(O)), np.clip(tr, -2.0, 2.0), act, k0, prev


@pytest.mark.parametrize('variant', ['cem', 'safe', 'cost'])
@pytest.mark.parametrize('shape', zc.SHAPES, ids=lambda s: 'O%d_A%d_H%d_rows%d_P%d' % s)
def test_kernel_equals_the_mirror(shape, variant):
    """Returns and cost bytes bit for bit, over a quadratic and a tracking base (the latter at a clock of (3, a non-zero action)):
    random states under six random zones (margins, penalties, a keep-in zone, unused slots) on top of the base task's crafted rows; the
    crafted zone rows (dist2 at exactly R2 and one ulp outside, keep-out and keep-in; inside the margin only; a NaN on an axis; a hit at
    s_0, at s_H, after near); sixteen active zones of mixed magnitude.  At O = 100 the crafted and the sixteen zones read the second
    quad.  Guard words behind both outputs stay; a 'cem' handle writes no cost byte.  The 16-byte shapes run a second time one float off
    alignment."""
    _torch()
    O, A, Hh, rows, Pp = shape
    pl = CemPlanner(tc.kernel_handle_config(O, A, Pp, variant))
    try:
        for kind in ('quadratic', 'tracking'):
            for name, task, tr, act, k0, prev in _kernel_cases(O, A, Hh, rows, Pp, kind):
                pl.set_task(task)
                assert pl.task_zones is task.zones
                if kind == 'tracking':
                    pl.set_task_clock(k0, prev)
                want_ret, want_costs = _objective(task, tr, act, variant, k0, prev)
                hit = zone_terms(tr, task.zone_tables(O))[0]
                assert rows < 9 or hit.any(), (kind, name)
                if name != 'sixteen' and rows > 8:                            # the zones matter: the base task says something else
                    assert not np.array_equal(want_ret, _objective(dataclasses.replace(task, zones=None), tr, act, variant, k0, prev)[0])
                for misalign in ([False, True] if O % 4 == 0 else [False]):
                    what = '%s %s (misalign %s)' % (kind, name, misalign)
                    ret, costs = _run_kernel(pl, tr, act, misalign)
                    _bits(ret, want_ret, 'returns, ' + what)
                    if variant == 'cem':
                        assert (costs == COST_GUARD).all()
                    else:
                        _bits(costs, want_costs, 'cost bytes, ' + what)
    finally:
        pl.close()


def test_idle_zones_and_cleared_zones_leave_the_kernels_bits():
    """Never-entered zero-penalty zones: cem_task_zones_kernel returns what the base task's kernel returns on a second handle, bit for
    bit, on every shape and both kinds; after the zones are cleared the handle IS the base task's again."""
    _torch()
    for (O, A, Hh, rows, Pp) in zc.SHAPES:
        for kind in ('quadratic', 'tracking'):
            base = tc.task_for(O, A, 0, True) if kind == 'quadratic' else tk.tracking_task_for(O, A, Hh + 1, 0, True)
            far = StateZones(axes=[[0, O - 1], [O - 1, 0]], centre=[[100.0, 100.0], [0.0, 0.0]], radius=[1.0, 1e3], margin=[1.0, 1.0],
                             penalty=[0.0, 5.0], keep_in=[0, 1])
            cfg = tc.kernel_handle_config(O, A, Pp, 'safe')
            a, b = CemPlanner(dataclasses.replace(cfg, task=base)), CemPlanner(dataclasses.replace(cfg, task=zc.with_zones(base, far)))
            try:
                tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
                if kind == 'quadratic':
                    tc.craft(tr, base)
                else:
                    prev = tk.prev_action_for(A)
                    tk.craft(tr, act, base, 1, prev)
                    a.set_task_clock(1, prev); b.set_task_clock(1, prev)
                ra, ca = _run_kernel(a, tr, act)
                rb, cb = _run_kernel(b, tr, act)
                _bits(rb, ra, 'returns, O %d %s' % (O, kind))
                _bits(cb, ca, 'cost bytes, O %d %s' % (O, kind))
                b.set_task_zones(None)
                assert b.task_zones is None
                rc_, cc_ = _run_kernel(b, tr, act)
                _bits(rc_, ra); _bits(cc_, ca)
            finally:
                a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# plans: N = 64, H = 10, P = 2, E = 2, two iterations
# ---------------------------------------------------------------------------------------------------------------------------------
_PROBLEM = []
T_PLAN = H + 4
PREV = np.array([0.25, -0.5], F)
K0 = 2


def _problem():
    if not _PROBLEM:
        _PROBLEM.append(hp.make_problem(obs_dim=60, act_dim=2, E=E, n_layers=4, seed=77))
    return _PROBLEM[0]


def _configs(variant='cem', I=2, **kw):
    pb = _problem()
    _, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=K, I=I, variant=variant, post=0.3, **kw)
    return pb, pcfg


def _run_all(pl, state, seed, call):
    """One stepwise plan to its end -> (per iteration: trajectories, actions, scores, returns, cost bytes), result."""
    per = []
    pl.plan_begin(state, seed, call)
    for it in range(pl.cfg.iterations):
        pl.plan_rollout(it)
        per.append(dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                        returns=_np(pl.returns()).reshape(-1), costs=_np(pl.costs()).reshape(-1)))
        pl.plan_select(it)
    return per, pl.plan_end()


def _calibrated_task(pl, pb, kind, idle=False):
    """A task whose zones are taken from the handle's own first rollout: three keep-out ellipses on feature pairs of 2 .. 7, centred
    where the rows are halfway through the plan, weighted by the inverse variances, each with the radius that a twentieth of the states after
    t = 0 lie within, a margin of half the radius and a penalty; a keep-in ellipsoid on features 8 .. 10 that a twentieth of the states
    leave.  idle: the same zones pushed out of reach with penalty 0.  (Thresholds of the TEST's task, not bars: every check below is bit
    for bit against the mirror on the device's own trajectories.)"""
    O = pb['state'].shape[0]
    pl.set_task(QuadraticTask(q=1.0, g=pb['state']))
    per, _ = _run_all(pl, pb['state'], SEED, 900)
    tr = per[0]['traj'].astype(np.float64)
    rng = np.random.default_rng(3)
    sd = tr[:, H // 2].std(axis=0)
    mid = tr[:, H // 2].mean(axis=0)
    axes, centre, weights, radius, keep_in = [], [], [], [], []
    for feats, kin, qt in (((2, 3), 0, 0.05), ((4, 5), 0, 0.05), ((6, 7), 0, 0.05), ((8, 9, 10), 1, 0.95)):
        f = list(feats)
        w = 1.0 / sd[f] ** 2
        c = mid[f] + (0.0 if kin else 0.5) * sd[f]
        d2 = (w * (tr[:, 1:, f] - c) ** 2).sum(axis=2)
        axes.append(f + [-1] * (4 - len(f))); centre.append(list(c) + [0.0] * (4 - len(f))); weights.append(list(w) + [0.0] * (4 - len(f)))
        radius.append(float(np.sqrt(np.quantile(d2, qt)))); keep_in.append(kin)
    radius = np.array(radius)
    zones = StateZones(axes=axes, centre=centre, weights=weights, radius=radius, margin=0.5 * radius, penalty=[0.5, 0.25, 1.0, 0.125], keep_in=keep_in)
    if idle:
        zones = dataclasses.replace(zones, centre=np.array(centre) + np.where(np.array(keep_in)[:, None] == 1, 0.0, 1e3),
                                    radius=np.where(np.array(keep_in) == 1, 1e4, radius), penalty=0.0)
    q = rng.uniform(0.0, 1.0, O).astype(F)
    m = np.zeros(O, F)
    m[:2] = 1.0
    lo, hi = np.full(O, -np.inf, F), np.full(O, np.inf, F)
    lo[12:14] = np.quantile(tr[:, 1:, 12:14], 0.05, axis=(0, 1))
    if kind == 'quadratic':
        g = pb['state'].astype(np.float64).copy()
        g[:2] += sd[:2]
        nsum = ((tr[:, :H, :2] - g[:2]) ** 2).sum(axis=2)
        task = QuadraticTask(q=q, g=g.astype(F), c=rng.normal(0, 0.01, O).astype(F), goal_mask=m, lo=lo, hi=hi, rho=[0.1, 0.2],
                             goal_radius=float(np.sqrt(np.median(nsum[:, 1:].min(axis=1)))), reward_goal=0.05, zones=zones)
    else:
        ref = pb['state'].astype(np.float64) + np.arange(T_PLAN)[:, None] * (0.05 * sd * rng.choice([-1.0, 1.0], O))
        ref[:, :2] += sd[:2]
        rows = ref[np.minimum(K0 + np.arange(H + 1), T_PLAN - 1)]
        nsum = ((tr[:, :H, :2] - rows[:H, :2]) ** 2).sum(axis=2)
        task = TrackingTask(reference=ref.astype(F), q=q, c=rng.normal(0, 0.01, O).astype(F), goal_mask=m, lo=lo, hi=hi, rho=[0.1, 0.2],
                            goal_radius=float(np.sqrt(np.median(nsum[:, 1:].min(axis=1)))), reward_goal=0.05,
                            terminal_weights=(4.0 * q).astype(F), action_rate=[0.3, 0.15], zones=zones)
    pl.set_task(task)
    if kind == 'tracking':
        pl.set_task_clock(K0, PREV)
    return task


def _planner(variant='cem', kind='quadratic', **kw):
    _torch()
    pb, pcfg = _configs(variant=variant, **kw)
    pl = hp.make_planner(pb, pcfg)
    return pb, pcfg, pl, _calibrated_task(pl, pb, kind)


def _clock(task):
    return (K0, PREV) if isinstance(task, TrackingTask) else (0, None)


def _restated_scores(variant, ret, costs, pcfg, n):
    r = ret.reshape(P, n)
    if variant == 'cem':
        return cc.mean_returns(r)
    cb = costs.reshape(H, P, n)
    if variant == 'cost':
        return cost_cases.scores_from_bytes(cb, P, n)
    unsafe = rk.unsafe_flags(cb, P, pcfg.posterior_mean_threashold)
    return cc.mean_returns(r) - np.where(unsafe, F(1.0), F(0.0)) * F(100.0)


def _check_iteration(rec, task, variant, pcfg, n=N, what=''):
    traj, act = rec['traj'][:P * n], rec['actions'][:n]
    ret, costs = _objective(task, traj, act, variant, *_clock(task))
    _bits(rec['returns'][:P * n], ret, '%s: returns' % what)
    if variant != 'cem':
        _bits(rec['costs'][:H * P * n].reshape(H, P * n), costs, '%s: cost bytes' % what)
    _bits(rec['scores'][:n], _restated_scores(variant, ret, costs, pcfg, n), '%s: scores' % what)
    return ret, costs


@pytest.mark.parametrize('variant,kind', [('cem', 'quadratic'), ('safe', 'tracking'), ('cost', 'quadratic'), ('cem', 'tracking')])
def test_scores_of_two_iterations_and_the_three_plan_forms(variant, kind):
    pb, pcfg, pl, task = _planner(variant=variant, kind=kind)
    others = []
    try:
        base_plan = None
        per, (a, s, iters) = _run_all(pl, pb['state'], SEED, 0)
        for it in range(2):
            ret, costs = _check_iteration(per[it], task, variant, pcfg, what='%s %s iteration %d' % (variant, kind, it))
            hit, pen, _ = zone_terms(per[it]['traj'], task.zone_tables(60))
            assert hit[:, :H].any() and not hit[:, :H].all() and (pen > 0).any() and not (pen > 0).all()      # the calibrated zones fall on both sides
            r0, c0 = _objective(dataclasses.replace(task, zones=None), per[it]['traj'], per[it]['actions'], variant, *_clock(task))
            assert not np.array_equal(r0, ret)                                  # the penalty reached the returns,
            assert variant == 'cem' or c0.sum() < costs.sum()                   # the hits the cost bytes
        assert not np.array_equal(per[0]['scores'], per[1]['scores'])
        assert pl.rollout_path() == 'generic'
        # eager and graph plans on handles of their own, Philox noise: the same action, score and iteration count
        for use_graph in (False, True):
            _, cfg2 = _configs(variant=variant, use_graph=use_graph)
            p2 = hp.make_planner(pb, dataclasses.replace(cfg2, task=task))
            others.append(p2)
            assert p2.task_zones is task.zones
            if kind == 'tracking':
                p2.set_task_clock(K0, PREV)
            for _ in range(2):                                     # (the second graph plan replays the captured one)
                a2, s2, i2 = p2.plan(pb['state'], seed=SEED, call=0)
                _bits(a2, a, 'action, use_graph %s' % use_graph)
                assert F(s2).view(U) == F(s).view(U) and i2 == iters
            assert p2.graph_status() == ('graph' if use_graph else 'eager')
            # recipe and launch count are the base task plan's
            base_plan = [p2.iteration_plan(i) for i in range(2)]
            nodes = p2.graph_nodes()
            p2.set_task_zones(None)
            assert [p2.iteration_plan(i) for i in range(2)] == base_plan
            if use_graph:
                p2.plan(pb['state'], seed=SEED, call=0)
                assert p2.graph_nodes() == nodes > 0
    finally:
        for p in [pl] + others:
            p.close()


@pytest.mark.parametrize('variant,kind', [('safe', 'quadratic'), ('cem', 'tracking')])
def test_idle_zones_and_cleared_zones_leave_every_result_bit_of_the_plan(variant, kind):
    """Three graph handles: the base task alone; the base task with zones that are never entered and have penalty 0; the base task with
    live zones that are cleared after a plan.  The second and the third (once cleared) give the first's action, score, returns, cost
    bytes and result block, with its iteration plan and graph node count."""
    _torch()
    pb, pcfg = _configs(variant=variant, use_graph=True)
    probe = hp.make_planner(pb, _configs(variant=variant)[1])
    try:
        live = _calibrated_task(probe, pb, kind)
        idle = _calibrated_task(probe, pb, kind, idle=True)
    finally:
        probe.close()
    base = dataclasses.replace(live, zones=None)
    never, idling, cleared = (hp.make_planner(pb, dataclasses.replace(pcfg, task=t)) for t in (base, idle, live))
    try:
        for p in (never, idling, cleared):
            if kind == 'tracking':
                p.set_task_clock(K0, PREV)
        a_live, _, _ = cleared.plan(pb['state'], seed=SEED, call=0)
        live_returns = _np(cleared.returns())
        cleared.set_task_zones(None)
        assert cleared.task_zones is None
        assert cleared.task_clock is None or cleared.task_clock[0] == K0       # (clearing the zones leaves the clock)
        for call in range(2):
            a, s, i = never.plan(pb['state'], seed=SEED, call=call)
            for p, what in ((idling, 'idle zones'), (cleared, 'cleared zones')):
                a2, s2, i2 = p.plan(pb['state'], seed=SEED, call=call)
                _bits(a2, a, what)
                assert F(s2).view(U) == F(s).view(U) and i2 == i, what
                _bits(_np(p.returns()), _np(never.returns()), what + ': returns')
                _bits(_np(p.costs()), _np(never.costs()), what + ': cost bytes')
                _bits(_np(p.result_block())[:36], _np(never.result_block())[:36], what + ': result block')
        assert not np.array_equal(live_returns, _np(never.returns()))
        plans = [[p.iteration_plan(i) for i in range(2)] for p in (never, idling, cleared)]
        assert plans[0] == plans[1] == plans[2]
        assert never.graph_status() == idling.graph_status() == cleared.graph_status() == 'graph'
        assert never.graph_nodes() == idling.graph_nodes() == cleared.graph_nodes() > 0
        # clearing twice is nothing: the graph stays
        cleared.set_task_zones(None)
        assert cleared.graph_status() == 'graph'
    finally:
        never.close(); idling.close(); cleared.close()


def test_the_clock_moves_and_the_graph_stays():
    """A tracking plan with zones, captured at the clock (K0, PREV); the clock moves to (K0 + 3, another action) between two decisions:
    the next plan replays the same graph and scores what the mirror scores at the new clock."""
    _torch()
    pb, pcfg = _configs(use_graph=True)
    probe = hp.make_planner(pb, _configs()[1])
    try:
        task = _calibrated_task(probe, pb, 'tracking')
    finally:
        probe.close()
    x = hp.make_planner(pb, dataclasses.replace(pcfg, task=task))
    try:
        x.set_task_clock(K0, PREV)
        x.plan(pb['state'], seed=SEED, call=0)
        x.plan(pb['state'], seed=SEED, call=1)
        assert x.graph_status() == 'graph'
        nodes, before = x.graph_nodes(), _np(x.returns())
        x.set_task_clock(K0 + 3, -PREV)
        x.plan(pb['state'], seed=SEED, call=1)
        assert x.graph_status() == 'graph' and x.graph_nodes() == nodes > 0
        ret, _ = tracking_objective(_np(x.task_trajectories()), _np(x.actions()), task, 'cem', k0=K0 + 3, prev_action=-PREV)
        _bits(_np(x.returns()).reshape(-1), ret, 'the last iteration of the replayed graph')
        assert not np.array_equal(_np(x.returns()), before)
    finally:
        x.close()


def test_with_risk_level():
    pb, pcfg, pl, task = _planner()
    try:
        pl.set_particle_objective('lower_tail', 2)
        per, _ = _run_all(pl, pb['state'], SEED, 0)
        ret, _ = task_objective(per[0]['traj'], per[0]['actions'], task, 'cem')
        _bits(per[0]['returns'], ret)
        _bits(per[0]['scores'], rk.scores(ret.reshape(P, N), 2), 'lower-tail scores')
    finally:
        pl.close()


def test_with_cost_budget():
    pb, pcfg, pl, task = _planner(variant='safe')
    try:
        pl.set_constraint('budget', 0)
        pl.set_cost_budget(3.0)
        per, _ = _run_all(pl, pb['state'], SEED, 0)
        ret, costs = task_objective(per[0]['traj'], per[0]['actions'], task, 'safe')
        want = cc.scores(ret.reshape(P, N), costs.reshape(H, P, N), P, N, P, 3.0)
        _bits(per[0]['scores'], want, 'budget scores')
        feas = cc.feasible(costs.reshape(H, P, N), P, N, P, 3.0)
        assert feas.any() and not feas.all()
        # the zones' hits are what makes candidates infeasible: the base task's bytes leave more of them feasible
        c0 = task_objective(per[0]['traj'], per[0]['actions'], dataclasses.replace(task, zones=None), 'safe')[1]
        assert cc.feasible(c0.reshape(H, P, N), P, N, P, 3.0).sum() > feas.sum()
    finally:
        pl.close()


def test_with_plan_readout():
    pb, pcfg, pl, task = _planner(variant='safe', I=1)
    try:
        pl.set_plan_readout(True)
        a, s, _ = pl.plan(pb['state'], seed=SEED, call=0)
        ro = pl.plan_readout()
        ret, costs = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'safe')
        assert ro.iteration == 0 and 0 <= ro.candidate < N
        _bits(ro.particle_returns, ret.reshape(P, N)[:, ro.candidate], 'particle returns of the winner')
        _bits(ro.sequence[0], a)
        # cost_counts counts zone hits: the particles of the winner with a non-zero byte per step, as the mirror has them
        counts = (costs.reshape(H, P, N)[:, :, ro.candidate] != 0).sum(axis=1).astype(np.int32)
        np.testing.assert_array_equal(ro.cost_counts, counts)
        # ... and over all candidates the mirror's bytes hold zone hits the base task does not have
        c0 = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), dataclasses.replace(task, zones=None), 'safe')[1]
        assert costs.sum() > c0.sum()
    finally:
        pl.close()


def test_with_a_population_schedule():
    pb, pcfg, pl, task = _planner(kind='tracking')
    n1 = 40
    try:
        pl.set_population_schedule([N, n1])
        assert pl.iteration_plan(1)['n_samples'] == n1 and pl.iteration_plan(1)['rollout_path'] == 'generic'
        pl.plan_begin(pb['state'], SEED, 0)
        for it, n in ((0, N), (1, n1)):
            pl.plan_rollout(it)
            rec = dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                       returns=_np(pl.returns()).reshape(-1), costs=None)
            _check_iteration(rec, task, 'cem', pcfg, n=n, what='iteration %d' % it)
            pl.plan_select(it)
        _, score, iters = pl.plan_end()
        assert np.isfinite(score) and iters == 2
    finally:
        pl.close()


def test_refusals():
    _torch()
    pb, pcfg = _configs()
    base = tc.task_for(60, 2)
    z = zc.random_zones(60)
    pl = hp.make_planner(pb, pcfg)
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)

    def call(n=1, axis=(0, 1, -1, -1), centre=(0.0,) * 4, weight=(1.0,) * 4, radius=1.0, margin=0.0, penalty=0.0, keep_in=0, drop=()):
        keep = dict(axis=np.array(list(axis) * max(n, 1), np.int32), centre=np.array(list(centre) * max(n, 1), F), weight=np.array(list(weight) * max(n, 1), F),
                    radius=np.full(max(n, 1), radius, F), margin=np.full(max(n, 1), margin, F), penalty=np.full(max(n, 1), penalty, F),
                    keep_in=np.full(max(n, 1), keep_in, np.int32))
        kw = {k: v.ctypes.data_as(ip if v.dtype == np.int32 else fp) for k, v in keep.items() if k not in drop}
        return pl.lib.cem_planner_set_task_zones(pl.h, C.byref(_capi.CemTaskZones(n_zones=n, **kw)))
    try:
        before = pl.iteration_plan(0)
        # no task in force: a state error; clearing nothing is nothing
        assert call() == STATE
        assert pl.lib.cem_planner_set_task_zones(pl.h, None) == 0
        with pytest.raises(_capi.CemError) as e:
            pl.set_task_zones(z)
        assert e.value.status == STATE
        pl.set_task(base)
        assert call() == 0 and call(n=16) == 0 and call(drop=('margin', 'penalty', 'keep_in')) == 0 and call(keep_in=1, margin=1.0) == 0
        bad = [dict(n=0), dict(n=17), dict(n=-1), dict(drop=('axis',)), dict(drop=('centre',)), dict(drop=('weight',)), dict(drop=('radius',)),
               dict(axis=(0, 60, -1, -1)), dict(axis=(0, -2, -1, -1)), dict(axis=(-1, -1, -1, -1)), dict(centre=(np.nan, 0, 0, 0)),
               dict(centre=(0, np.inf, 0, 0)), dict(weight=(-1.0, 1, 1, 1)), dict(weight=(np.nan, 1, 1, 1)), dict(radius=0.0), dict(radius=-1.0),
               dict(radius=np.nan), dict(radius=np.inf), dict(margin=-0.5), dict(margin=np.nan), dict(penalty=-1.0), dict(penalty=np.inf),
               dict(keep_in=1, margin=1.5), dict(keep_in=2), dict(keep_in=-1)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, kw
        # an unused slot's centre and weight are not read
        assert call(centre=(0, 0, np.nan, np.nan), weight=(1, 1, -1, np.nan), margin=0.5, penalty=2.0) == 0
        # a refused call left the zones of the last good one: one zone on features 0 and 1
        tr, act = tc.random_case(60, 2, 7, 2 * P, P, 0)
        t = _torch()
        want = task_objective(tr, act, zc.with_zones(base, StateZones(axes=[[0, 1]], centre=0.0, radius=1.0, margin=0.5, penalty=2.0)), 'cem')[0]
        got, _ = pl.task_score(t.from_numpy(tr), t.from_numpy(act))
        _bits(_np(got), want)
        # set_task clears them; the Python task sets both
        pl.set_task(base)
        assert pl.task_zones is None and pl.iteration_plan(0)['launches'] > before['launches']
        _bits(_np(pl.task_score(t.from_numpy(tr), t.from_numpy(act))[0]), task_objective(tr, act, base, 'cem')[0])
        pl.set_task(zc.with_zones(base, z))
        assert pl.task_zones is z
        # a task whose zones are refused is refused before anything changes
        with pytest.raises(ValueError):
            pl.set_task(zc.with_zones(base, dataclasses.replace(z, radius=-1.0)))
        assert pl.task_zones is z
        # inside a stepwise plan
        pl.plan_begin(pb['state'], SEED, 0)
        assert call() == STATE and pl.lib.cem_planner_set_task_zones(pl.h, None) == STATE
        for it in range(pcfg.iterations):
            pl.plan_rollout(it); pl.plan_select(it)
        pl.plan_end()
        pl.set_task(None)
        assert call() == STATE and pl.iteration_plan(0) == before
    finally:
        pl.close()
    # a batch handle and a sharded one still refuse the task, zones or none
    bp = BatchCemPlanner(pcfg, 2)
    try:
        with pytest.raises(_capi.CemError) as e:
            bp.set_task(zc.with_zones(base, z))
        assert e.value.status == UNSUPPORTED
    finally:
        bp.close()
    _, cfg_w = _configs(world_size=2)
    pw = CemPlanner(cfg_w)
    try:
        with pytest.raises(_capi.CemError) as e:
            pw.set_task(zc.with_zones(base, z))
        assert e.value.status == UNSUPPORTED
    finally:
        pw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the closed loop: a point mass goes round a disc
# ---------------------------------------------------------------------------------------------------------------------------------
def _point_mass_policy(task, cls=None, **kw):
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    c = zc.LOOP
    box = lambda lo, hi: types.SimpleNamespace(low=np.asarray(lo, F), high=np.asarray(hi, F), shape=(len(lo),))
    obs_space, act_space = box([-10.0] * 4, [10.0] * 4), box([-1.0, -1.0], [1.0, 1.0])
    model = TransitionModel('mlp_ensemble', obs_space, act_space, scale_features=False, sampling_propagation=False, ensemble_size=c['E'],
                            mlp_params=dict(n_layers=2, units=zc.UNITS, activation='tf.nn.relu', dropout_rate=0.0))
    model.model.set_weights(zc.point_mass_weights(c['E']))
    env = types.SimpleNamespace(action_space=act_space, observation_space=obs_space)
    return (cls or CemMpc)(model=model, environment=env, horizon=c['H'], iterations=c['I'], smoothing=0.0, n_samples=c['N'], n_elite=c['k'],
                           particles=c['P'], stddev_threshold=-1.0, noise_stddev=0.0, seed=SEED, task=task, **kw)


def _drive(pol, check=None):
    s = zc.START.copy()
    executed = []
    for step in range(zc.LOOP['steps']):
        a = pol.generate_action(s)
        if check is not None and step == 9:
            check(pol)
        s = zc.point_mass_step(s, a[:2])
        executed.append(s.copy())
    return s, np.array(executed)


def test_closed_loop_goes_round_the_disc():
    """CemMpc(task=QuadraticTask(..., zones=a disc)) drives a point mass (the ensemble set by hand to its exact dynamics, model noise
    off) from (-1, 0.02) at rest to (1, 0): N = 64, H = 12, I = 4, k = 6, P = 2, 80 decisions; a keep-out disc of radius 0.3 at the
    origin with a margin of 0.3 and a penalty of 30 lies across the straight line.  The yardstick is a NumPy CEM on the same model scored
    by the mirror (zone_cases.reference_closed_loop), seeds 0 .. 4, measured on the CPU: it never executes a state inside the disc, its
    worst final stage cost is 5.99e-4, and without the zones it runs through the disc (5 states inside on every seed).  The policy
    executes no state inside the disc and ends within 2 x 5.99e-4 of the set-point."""
    _torch()
    task = zc.loop_task('penalty')

    def check(pol):
        pl = pol._planner
        assert pl.task_zones is task.zones and pl.rollout_path() == 'generic'
        ret, _ = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'cem')
        _bits(_np(pl.returns()).reshape(-1), ret, 'returns of decision 9')
    s, executed = _drive(_point_mass_policy(task), check)
    inside, cost = zc.inside_disc(executed), zc.stage_cost(s)
    closest = float(np.sqrt((executed[:, :2].astype(np.float64) ** 2).sum(axis=1)).min())
    print('round the disc: %d states inside, closest %.3f (radius %.1f), final stage cost %.3g (reference worst %.3g)'
          % (inside, closest, zc.DISC_RADIUS, cost, zc.REFERENCE_WORST_STAGE_COST))
    assert inside == 0
    assert cost <= 2 * zc.REFERENCE_WORST_STAGE_COST, cost


def test_closed_loop_the_beta_filter_keeps_out_of_the_bare_disc():
    """SafeCemMpc with the bare disc (penalty 0: the zone only sets cost bytes, the Beta filter does the rest): no executed state
    inside."""
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    _torch()
    task = zc.loop_task('hits')

    def check(pol):
        pl = pol._planner
        ret, costs = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'safe')
        _bits(_np(pl.costs()).reshape(-1), costs.reshape(-1), 'cost bytes of decision 9')
    s, executed = _drive(_point_mass_policy(task, SafeCemMpc, posterior_mean_threashold=0.3), check)
    inside = zc.inside_disc(executed)
    closest = float(np.sqrt((executed[:, :2].astype(np.float64) ** 2).sum(axis=1)).min())
    print('round the bare disc: %d states inside, closest %.3f (radius %.1f), final stage cost %.3g' % (inside, closest, zc.DISC_RADIUS, zc.stage_cost(s)))
    assert inside == 0
