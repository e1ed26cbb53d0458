"""Linear outputs on a task (cem_planner_set_task_outputs) on the device.

The kernel has an exact reference that costs nothing: planner.task_objective / tracking_objective restate cem_task_outputs_kernel bit
for bit (tests/test_outputs_cpu.py holds that mirror to a float64 statement of the contract).  So (1) the kernel alone is held to the
mirror on random and crafted tensors over both base kinds, (2) a plan's returns, cost bytes and scores to the mirror on the trajectories
the handle itself kept, in every plan form, (3) outputs that do nothing and outputs that were cleared are shown to leave the base task's
bits, and the rest — the other options, the refusals, the two closed loops — hangs off that."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner, StateZones, TaskOutputs, _capi
from ethz_safe_learning_amd.planner import QuadraticTask, TrackingTask, output_terms, task_objective, tracking_objective
from tests import constrained_cases as cc
from tests import cost_cases
from tests import helpers as hp
from tests import output_cases as oc
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
    """(name, task, traj, actions, k0, prev): random states under M = 1, 7, 16 random outputs over the base task's own crafted rows, with
    zones on output axes for M = 1 and 16 and without for M = 7, a per-step target on the tracking base; the crafted rows; sixteen
    outputs of mixed magnitude on a base task without weights (O >= 57)."""
    if kind == 'quadratic':
        base, k0, prev = tc.task_for(O, A, 0, True), 0, None
    else:
        base, k0, prev = tk.tracking_task_for(O, A, Hh + 1, 0, True), 3, tk.prev_action_for(A)
    tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
    if kind == 'quadratic':
        tc.craft(tr, base)
    else:
        tk.craft(tr, act, base, k0, prev)
    for M in oc.COUNTS:
        out = oc.random_outputs(O, M, 0, T=Hh + 1 if kind == 'tracking' else None, terminal=kind == 'tracking')
        yield 'random M=%d' % M, oc.with_outputs(base, out, oc.output_zones(O, M) if M != 7 else None), tr, act, k0, prev
    if O >= 57:
        cbase, g, ck0, cprev = zc.crafted_base(O, A, kind, Hh)
        task, ctr, cact, _ = oc.crafted_case(cbase, O, A, Hh, Pp, g)
        yield 'crafted', task, ctr, cact, ck0, cprev
        plain = dataclasses.replace(base, q=0.0, c=0.0, **({'terminal_weights': None} if kind == 'tracking' else {}))
        yield 'sixteen', oc.with_outputs(plain, oc.sixteen_outputs(O)), np.clip(tr, -2.0, 2.0), act, k0, prev


@pytest.mark.parametrize('variant', ['cem', 'safe', 'cost'])
@pytest.mark.parametrize('shape', oc.SHAPES, ids=lambda s: 'O%d_A%d_H%d_rows%d_P%d' % s)
def test_kernel_equals_the_mirror(shape, variant):
    """Returns and cost bytes bit for bit, over a quadratic and a tracking base (the latter at a clock of (3, a non-zero action) with a
    per-step target of the outputs and terminal weights): M = 1, 7 and 16 random outputs (at O = 100 with entries on features >= 64),
    with and without zones that name outputs; the crafted rows (an output exactly on hi and one ulp outside; near at exactly R2 through
    the output's near weight alone; a terminal weight; a NaN feature under a zero column; a zone on two outputs at exactly R2 and one ulp
    outside; a violation at s_0, at s_H, after near); sixteen output slots six decades apart.  Guard words behind both results stay; a
    'cem' handle writes no cost byte.  The 16-byte shapes run a second time one float off alignment."""
    _torch()
    O, A, Hh, rows, Pp = shape
    pl = CemPlanner(tc.kernel_handle_config(O, A, Pp, variant))
    try:
        for kind in ('quadratic', 'tracking'):
            for name, task, tr, act, k0, prev in _kernel_cases(O, A, Hh, rows, Pp, kind):
                pl.set_task(task)
                assert pl.task_outputs is task.outputs and pl.task_zones is task.zones
                if kind == 'tracking':
                    pl.set_task_clock(k0, prev)
                want_ret, want_costs = _objective(task, tr, act, variant, k0, prev)
                if rows > 8:                                                   # the outputs matter: the base task says something else
                    bare = _objective(dataclasses.replace(task, outputs=None, zones=None), tr, act, variant, k0, prev)
                    assert not np.array_equal(want_ret, bare[0]), (kind, name)
                    assert variant == 'cem' or name == 'sixteen' or want_costs.sum() > bare[1].sum(), (kind, name)
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


def _idle(O, M):
    rng = np.random.default_rng(M)
    return TaskOutputs(matrix=rng.uniform(-1.0, 1.0, (M, O)).astype(F), target=rng.normal(0.0, 1.0, M).astype(F))


def test_idle_outputs_and_cleared_outputs_leave_the_kernels_bits():
    """Outputs with no weight, no linear term, no near weight and infinite bounds: cem_task_outputs_kernel returns what the base task's
    kernel returns on a second handle, bit for bit, on every shape and both kinds; after the outputs are cleared the handle IS the base
    task's again."""
    _torch()
    for (O, A, Hh, rows, Pp) in oc.SHAPES:
        for kind, M in (('quadratic', 16), ('tracking', 7)):
            base = tc.task_for(O, A, 0, True) if kind == 'quadratic' else tk.tracking_task_for(O, A, Hh + 1, 0, True)
            cfg = tc.kernel_handle_config(O, A, Pp, 'safe')
            a, b = CemPlanner(dataclasses.replace(cfg, task=base)), CemPlanner(dataclasses.replace(cfg, task=oc.with_outputs(base, _idle(O, M))))
            try:
                tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
                if kind == 'quadratic':
                    tc.craft(tr, base, boundaries=False)
                else:
                    prev = tk.prev_action_for(A)
                    tk.craft(tr, act, base, 1, prev, boundaries=False)
                    a.set_task_clock(1, prev); b.set_task_clock(1, prev)
                ra, ca = _run_kernel(a, tr, act)
                rb, cb = _run_kernel(b, tr, act)
                _bits(rb, ra, 'returns, O %d %s' % (O, kind))
                _bits(cb, ca, 'cost bytes, O %d %s' % (O, kind))
                b.set_task_outputs(None)
                assert b.task_outputs is None
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
M_PLAN = 5


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
    """A task whose outputs are taken from the handle's own first rollout: five random combinations of the state, weighted by their
    inverse variances towards their means (a per-step target on a tracking base), bounded where a twentieth of the states after t = 0
    lie beyond, and a keep-out ellipse on outputs 0 and 1 with the radius a twentieth of those states lie within, a margin and a
    penalty.  idle: the same matrix with nothing else.  (Thresholds of the TEST's task, not bars: every check below is bit for bit against
    the mirror on the device's own trajectories.)"""
    O = pb['state'].shape[0]
    pl.set_task(QuadraticTask(q=1.0, g=pb['state']))
    per, _ = _run_all(pl, pb['state'], SEED, 900)
    tr = per[0]['traj'].astype(np.float64)
    rng = np.random.default_rng(3)
    Cm = rng.uniform(-1.0, 1.0, (M_PLAN, O)).astype(F)
    y = tr[:, 1:] @ Cm.astype(np.float64).T
    sd, mid = y.std(axis=(0, 1)), y.mean(axis=(0, 1))
    lo, hi = np.full(M_PLAN, -np.inf), np.full(M_PLAN, np.inf)
    hi[2], lo[3] = np.quantile(y[..., 2], 0.95), np.quantile(y[..., 3], 0.05)
    zc_ = mid[:2] + 0.5 * sd[:2]
    d2 = (((y[..., :2] - zc_) / sd[:2]) ** 2).sum(axis=2)
    radius = float(np.sqrt(np.quantile(d2, 0.05)))
    zones = StateZones(axes=[[O, O + 1]], centre=[zc_], weights=[1.0 / sd[:2] ** 2], radius=radius, margin=0.5 * radius, penalty=0.5)
    target = mid if kind == 'quadratic' else mid + 0.1 * sd * np.arange(T_PLAN)[:, None]
    outs = TaskOutputs(matrix=Cm, weights=0.2 / sd ** 2, target=target.astype(F), linear=rng.normal(0, 0.01, M_PLAN).astype(F), lo=lo, hi=hi,
                       terminal_weights=(0.8 / sd ** 2) if kind == 'tracking' else None)
    if idle:
        outs, zones = TaskOutputs(matrix=Cm, target=target.astype(F)), None
    sdx = tr[:, H // 2].std(axis=0)
    q = rng.uniform(0.0, 1.0, O).astype(F)
    m = np.zeros(O, F)
    m[:2] = 1.0
    if kind == 'quadratic':
        g = pb['state'].astype(np.float64).copy()
        g[:2] += sdx[:2]
        nsum = ((tr[:, :H, :2] - g[:2]) ** 2).sum(axis=2)
        task = QuadraticTask(q=q, g=g.astype(F), goal_mask=m, rho=[0.1, 0.2], goal_radius=float(np.sqrt(np.median(nsum[:, 1:].min(axis=1)))),
                             reward_goal=0.05, outputs=outs, zones=zones)
    else:
        ref = pb['state'].astype(np.float64) + np.arange(T_PLAN)[:, None] * (0.05 * sdx * rng.choice([-1.0, 1.0], O))
        ref[:, :2] += sdx[:2]
        rows = ref[np.minimum(K0 + np.arange(H + 1), T_PLAN - 1)]
        nsum = ((tr[:, :H, :2] - rows[:H, :2]) ** 2).sum(axis=2)
        task = TrackingTask(reference=ref.astype(F), q=q, goal_mask=m, rho=[0.1, 0.2], goal_radius=float(np.sqrt(np.median(nsum[:, 1:].min(axis=1)))),
                            reward_goal=0.05, terminal_weights=(4.0 * q).astype(F), action_rate=[0.3, 0.15], outputs=outs, zones=zones)
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
        per, (a, s, iters) = _run_all(pl, pb['state'], SEED, 0)
        for it in range(2):
            ret, costs = _check_iteration(per[it], task, variant, pcfg, what='%s %s iteration %d' % (variant, kind, it))
            r0, c0 = _objective(dataclasses.replace(task, outputs=None, zones=None), per[it]['traj'], per[it]['actions'], variant, *_clock(task))
            assert not np.array_equal(r0, ret)                                  # the outputs reached the returns,
            assert variant == 'cem' or c0.sum() < costs.sum() < costs.size      # their bounds and the zone on them the cost bytes
        assert not np.array_equal(per[0]['scores'], per[1]['scores'])
        assert pl.rollout_path() == 'generic'
        # eager and graph plans on handles of their own, Philox noise: the same action, score and iteration count
        for use_graph in (False, True):
            _, cfg2 = _configs(variant=variant, use_graph=use_graph)
            p2 = hp.make_planner(pb, dataclasses.replace(cfg2, task=task))
            others.append(p2)
            assert p2.task_outputs is task.outputs and p2.task_zones is task.zones
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
            p2.set_task_outputs(None)
            assert p2.task_outputs is None and p2.task_zones is None
            assert [p2.iteration_plan(i) for i in range(2)] == base_plan
            if use_graph:
                p2.plan(pb['state'], seed=SEED, call=0)
                assert p2.graph_nodes() == nodes > 0
    finally:
        for p in [pl] + others:
            p.close()


@pytest.mark.parametrize('variant,kind', [('safe', 'quadratic'), ('cem', 'tracking')])
def test_idle_outputs_and_cleared_outputs_leave_every_result_bit_of_the_plan(variant, kind):
    """Three graph handles: the base task alone; the base task with outputs that weigh nothing and bound nothing; the base task with live
    outputs that are cleared after a plan.  The second and the third (once cleared) give the first's action, score, returns, cost bytes
    and result block, with its iteration plan and graph node count."""
    _torch()
    pb, pcfg = _configs(variant=variant, use_graph=True)
    probe = hp.make_planner(pb, _configs(variant=variant)[1])
    try:
        live = _calibrated_task(probe, pb, kind)
        idle = _calibrated_task(probe, pb, kind, idle=True)
    finally:
        probe.close()
    base = dataclasses.replace(live, outputs=None, zones=None)
    never, idling, cleared = (hp.make_planner(pb, dataclasses.replace(pcfg, task=t)) for t in (base, idle, live))
    try:
        for p in (never, idling, cleared):
            if kind == 'tracking':
                p.set_task_clock(K0, PREV)
        cleared.plan(pb['state'], seed=SEED, call=0)
        live_returns = _np(cleared.returns())
        cleared.set_task_outputs(None)
        assert cleared.task_outputs is None and cleared.task_zones is None
        assert cleared.task_clock is None or cleared.task_clock[0] == K0       # (clearing the outputs leaves the clock)
        for call in range(2):
            a, s, i = never.plan(pb['state'], seed=SEED, call=call)
            for p, what in ((idling, 'idle outputs'), (cleared, 'cleared outputs')):
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
        cleared.set_task_outputs(None)                                          # clearing twice is nothing: the graph stays
        assert cleared.graph_status() == 'graph'
    finally:
        never.close(); idling.close(); cleared.close()


def test_the_clock_moves_and_the_graph_stays():
    """A tracking plan with outputs on a per-step target, captured at the clock (K0, PREV); the clock moves between two decisions: the
    next plan replays the same graph and scores what the mirror scores at the new clock."""
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
        # the outputs' bounds are what makes candidates infeasible: the base task has no cost at all
        feas = cc.feasible(costs.reshape(H, P, N), P, N, P, 3.0)
        c0 = task_objective(per[0]['traj'], per[0]['actions'], dataclasses.replace(task, outputs=None, zones=None), 'safe')[1]
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
        counts = (costs.reshape(H, P, N)[:, :, ro.candidate] != 0).sum(axis=1).astype(np.int32)
        np.testing.assert_array_equal(ro.cost_counts, counts)
        assert costs.sum() > 0
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
    outs = oc.random_outputs(60, 3)
    pl = hp.make_planner(pb, pcfg)
    fp = C.POINTER(C.c_float)

    def call(n=2, ref_rows=0, drop=(), **over):
        m = max(n, 1)
        keep = dict(matrix=np.ones((m, 60), F), weight=np.zeros(m, F), target=np.zeros(m, F), linear=np.zeros(m, F), near=np.zeros(m, F),
                    lo=np.full(m, -1.0, F), hi=np.full(m, 1.0, F), terminal=np.zeros(m, F))
        if ref_rows:
            keep['reference'] = np.zeros((ref_rows, m), F)
        for k, v in over.items():
            keep[k] = np.array(keep[k]); keep[k].reshape(-1)[0] = v
        kw = {k: v.ctypes.data_as(fp) for k, v in keep.items() if k not in drop}
        return pl.lib.cem_planner_set_task_outputs(pl.h, C.byref(_capi.CemTaskOutputs(n_outputs=n, ref_rows=ref_rows, **kw)))

    def zone(axis):
        ax = np.array(axis, np.int32)
        ones = np.ones(4, F)
        z = _capi.CemTaskZones(n_zones=1, axis=ax.ctypes.data_as(C.POINTER(C.c_int32)), centre=ones.ctypes.data_as(fp), weight=ones.ctypes.data_as(fp),
                               radius=ones.ctypes.data_as(fp))
        return pl.lib.cem_planner_set_task_zones(pl.h, C.byref(z))
    try:
        before = pl.iteration_plan(0)
        # no task in force: a state error; clearing nothing is nothing
        assert call() == STATE
        assert pl.lib.cem_planner_set_task_outputs(pl.h, None) == 0
        assert pl.lib.cem_planner_set_task_outputs(None, None) == INVALID_ARG
        with pytest.raises(_capi.CemError) as e:
            pl.set_task_outputs(outs)
        assert e.value.status == STATE
        pl.set_task(base)
        # a zone axis >= obs_dim without outputs is refused as it was
        assert zone([0, 60, -1, -1]) == INVALID_ARG
        assert call() == 0 and call(n=16) == 0 and call(n=1, ref_rows=1) == 0
        assert call(drop=('weight', 'target', 'linear', 'near', 'lo', 'hi', 'terminal')) == 0
        bad = [dict(n=0), dict(n=17), dict(n=-1), dict(drop=('matrix',)), dict(matrix=np.nan), dict(matrix=np.inf), dict(weight=-1.0), dict(weight=np.nan),
               dict(target=np.inf), dict(linear=np.nan), dict(near=np.inf), dict(terminal=-1.0), dict(terminal=np.nan), dict(lo=np.nan), dict(hi=np.nan),
               dict(lo=2.0), dict(ref_rows=2)]
        for kw in bad:
            assert call(**kw) == INVALID_ARG, kw
        assert call(lo=-np.inf, hi=np.inf) == 0
        # with two outputs in force a zone may name 60 and 61, not 62; the outputs' setter clears the zones
        assert zone([60, 61, -1, -1]) == 0 and zone([0, 62, -1, -1]) == INVALID_ARG
        assert call() == 0
        # a refused call left the outputs of the last good one: two outputs that sum the state, bounded by +-1, and no zone
        tr, act = tc.random_case(60, 2, 7, 2 * P, P, 0)
        t = _torch()
        kept = oc.with_outputs(base, TaskOutputs(matrix=np.ones((2, 60), F), lo=-1.0, hi=1.0))
        got, _ = pl.task_score(t.from_numpy(tr), t.from_numpy(act))
        _bits(_np(got), task_objective(tr, act, kept, 'cem')[0])
        # set_task clears them; the Python task sets both
        pl.set_task(base)
        assert pl.task_outputs is None and pl.iteration_plan(0)['launches'] > before['launches']
        _bits(_np(pl.task_score(t.from_numpy(tr), t.from_numpy(act))[0]), task_objective(tr, act, base, 'cem')[0])
        assert zone([0, 60, -1, -1]) == INVALID_ARG
        full = oc.with_outputs(base, outs, oc.output_zones(60, 3))
        pl.set_task(full)
        assert pl.task_outputs is outs and pl.task_zones is full.zones
        # a task whose outputs or zones are refused is refused before anything changes
        with pytest.raises(ValueError):
            pl.set_task(oc.with_outputs(base, dataclasses.replace(outs, weights=-1.0)))
        with pytest.raises(ValueError):
            pl.set_task(oc.with_outputs(base, outs, StateZones(axes=[[0, 63]], radius=1.0)))
        assert pl.task_outputs is outs
        # a per-step target needs a tracking base with as many rows
        with pytest.raises(ValueError):
            pl.set_task(oc.with_outputs(base, dataclasses.replace(outs, target=np.zeros((4, 3), F))))
        # inside a stepwise plan
        pl.plan_begin(pb['state'], SEED, 0)
        assert call() == STATE and pl.lib.cem_planner_set_task_outputs(pl.h, None) == STATE
        for it in range(pcfg.iterations):
            pl.plan_rollout(it); pl.plan_select(it)
        pl.plan_end()
        pl.set_task(None)
        assert call() == STATE and pl.iteration_plan(0) == before
    finally:
        pl.close()
    # a batch handle and a sharded one still refuse the task, outputs or none
    bp = BatchCemPlanner(pcfg, 2)
    try:
        with pytest.raises(_capi.CemError) as e:
            bp.set_task(oc.with_outputs(base, outs))
        assert e.value.status == UNSUPPORTED
        assert bp.lib.cem_planner_set_task_outputs(bp.h, C.byref(_capi.CemTaskOutputs(n_outputs=1, matrix=np.ones(60, F).ctypes.data_as(fp)))) == STATE
    finally:
        bp.close()
    _, cfg_w = _configs(world_size=2)
    pw = CemPlanner(cfg_w)
    try:
        with pytest.raises(_capi.CemError) as e:
            pw.set_task(oc.with_outputs(base, outs))
        assert e.value.status == UNSUPPORTED
    finally:
        pw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the closed loops: a point mass at a slanted wall and at a thin diagonal obstacle
# ---------------------------------------------------------------------------------------------------------------------------------
def _point_mass_policy(task, cls=None, **kw):
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    c = oc.LOOP
    box = lambda lo, hi: types.SimpleNamespace(low=np.asarray(lo, F), high=np.asarray(hi, F), shape=(len(lo),))
    obs_space, act_space = box([-10.0] * 4, [10.0] * 4), box([-1.0, -1.0], [1.0, 1.0])
    model = TransitionModel('mlp_ensemble', obs_space, act_space, scale_features=False, sampling_propagation=False, ensemble_size=c['E'],
                            mlp_params=dict(n_layers=2, units=zc.UNITS, activation='tf.nn.relu', dropout_rate=0.0))
    model.model.set_weights(zc.point_mass_weights(c['E']))
    env = types.SimpleNamespace(action_space=act_space, observation_space=obs_space)
    return (cls or CemMpc)(model=model, environment=env, horizon=c['H'], iterations=c['I'], smoothing=0.0, n_samples=c['N'], n_elite=c['k'],
                           particles=c['P'], stddev_threshold=-1.0, noise_stddev=0.0, seed=SEED, task=task, **kw)


def _drive(pol, check=None):
    s = oc.START.copy()
    executed = []
    for step in range(oc.LOOP['steps']):
        a = pol.generate_action(s)
        if check is not None and step == 9:
            check(pol)
        s = zc.point_mass_step(s, a[:2])
        executed.append(s.copy())
    return s, np.array(executed)


def test_closed_loop_stops_at_the_half_space():
    """SafeCemMpc drives zone_cases' point mass from (-1, 0.02) at rest towards (1, 0), which lies behind the wall (x + y) / sqrt(2) <=
    0.3: N = 64, H = 12, I = 4, 80 decisions.  The wall is the bound of one output (a cost byte beyond it: the Beta filter's business)
    and, in front of it, a keep-in zone on the same output with a margin of 0.15 and a penalty of 10.  The yardstick is a NumPy CEM on
    the same model scored by the mirror (output_cases.reference_closed_loop), seeds 0 .. 4, measured on the CPU: it executes no state
    beyond the wall and ends within 0.169 of the wall's closest point to the target, (0.712, -0.288); without the outputs it crosses the
    wall on every seed.  The policy executes no state beyond the wall and ends within 2 x 0.169 of that point."""
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    _torch()
    task = oc.wall_task(True)

    def check(pol):
        pl = pol._planner
        assert pl.task_outputs is task.outputs and pl.task_zones is task.zones and pl.rollout_path() == 'generic'
        ret, costs = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'safe')
        _bits(_np(pl.returns()).reshape(-1), ret, 'returns of decision 9')
        _bits(_np(pl.costs()).reshape(-1), costs.reshape(-1), 'cost bytes of decision 9')
    s, executed = _drive(_point_mass_policy(task, SafeCemMpc, posterior_mean_threashold=0.3), check)
    beyond = oc.beyond_wall(executed)
    dist = float(np.linalg.norm(s[:2].astype(np.float64) - oc.CLOSEST))
    print('at the wall: %d states beyond, final (%.3f, %.3f), %.3f from (%.3f, %.3f) (reference worst %.3f)'
          % (beyond, s[0], s[1], dist, oc.CLOSEST[0], oc.CLOSEST[1], oc.REFERENCE_WALL_WORST_DISTANCE))
    assert beyond == 0
    assert dist <= 2 * oc.REFERENCE_WALL_WORST_DISTANCE, dist


def test_closed_loop_goes_round_the_rotated_zone():
    """CemMpc with outputs u = (x + y) / sqrt(2), v = (y - x) / sqrt(2) and a keep-out zone on (u, v) with weights (1, 25) and radius
    0.5 — a thin diagonal obstacle across the straight line — a margin of 0.25 and a penalty of 30.  The NumPy CEM executes no state
    inside on seeds 0 .. 4 with a worst final stage cost of 1.16e-3, and runs through the obstacle on every seed without the outputs.
    The policy executes no state inside and ends within 2 x 1.16e-3 of the set-point."""
    _torch()
    task = oc.zone_task(True)

    def check(pol):
        pl = pol._planner
        assert pl.task_outputs is task.outputs and pl.task_zones is task.zones
        ret, _ = task_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'cem')
        _bits(_np(pl.returns()).reshape(-1), ret, 'returns of decision 9')
    s, executed = _drive(_point_mass_policy(task), check)
    inside, cost = oc.inside_zone(executed), zc.stage_cost(s)
    print('round the rotated zone: %d states inside, final stage cost %.3g (reference worst %.3g)' % (inside, cost, oc.REFERENCE_ZONE_WORST_STAGE_COST))
    assert inside == 0
    assert cost <= 2 * oc.REFERENCE_ZONE_WORST_STAGE_COST, cost
