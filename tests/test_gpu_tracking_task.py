"""The tracking task (cem_planner_set_task_tracking, cem_planner_set_task_clock) on the device.

As with the quadratic task, the kernel has an exact reference that costs nothing: planner.tracking_objective restates it bit for bit
(tests/test_tracking_cpu.py holds that mirror to a float64 statement of the contract).  So (1) the kernel alone is held to the mirror
on random and crafted tensors under every kind of clock, (2) a plan's returns, cost bytes and scores to the mirror on the trajectories
the handle itself kept, in every plan form, (3) the clock is shown to reach a captured plan without re-capturing it, and the rest — the
other options, off is off, the refusals, the policy's clock, a closed loop that follows a sine — hangs off that."""
import ctypes as C
import dataclasses
import types

import numpy as np
import pytest

from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner, _capi
from ethz_safe_learning_amd.planner import QuadraticTask, TrackingTask, task_objective, tracking_objective
from tests import constrained_cases as cc
from tests import cost_cases
from tests import helpers as hp
from tests import risk_cases as rk
from tests import task_cases as tc
from tests import tracking_cases as tk

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
@pytest.mark.parametrize('shape', tk.SHAPES, ids=lambda s: 'O%d_A%d_H%d_rows%d_P%d' % s)
def test_kernel_equals_the_mirror(shape, variant):
    """Returns and cost bytes bit for bit under the five clocks of tracking_cases.clock_cases (one row; a row per state; the last three
    states on the last row; a short table; every state on the last row), with terminal weights, an action rate and a non-zero previous
    action: random rows and the crafted ones (on a bound, one ulp outside, near at exactly R2 of a moving row and one ulp outside, the
    goal at t = 0 / at the last step / never, a NaN feature, one deviation at s_H and the same at s_{H-1}, a first action that equals
    the previous one), the reward clip active on about half of the steps; guard words behind both outputs stay; a 'cem' handle writes no
    cost byte.  The 16-byte shapes run a second time one float off alignment."""
    _torch()
    O, A, Hh, rows, Pp = shape
    pl = CemPlanner(tc.kernel_handle_config(O, A, Pp, variant))
    prev = tk.prev_action_for(A)
    try:
        for T, k0 in tk.clock_cases(Hh):
            task = tk.tracking_task_for(O, A, T, 0, True)
            pl.set_task(task)
            assert pl.task_clock[0] == 0 and not pl.task_clock[1].any()
            pl.set_task_clock(k0, prev)
            tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
            names = tk.craft(tr, act, task, k0, prev)
            want_ret, want_costs, first = tracking_objective(tr, act, task, variant, k0=k0, prev_action=prev, return_done=True)
            if rows > 12 and Hh >= 3:
                assert {'on_bounds', 'ulp_below_lo', 'near_exactly', 'near_ulp_outside', 'goal_at_0', 'goal_at_last_step', 'goal_never', 'nan_feature',
                        'deviation_at_H', 'deviation_before_H', 'first_action_is_previous'} <= set(names)
                assert first[names['near_exactly']] == names['near_state'] and first[names['near_ulp_outside']] == Hh
                assert (first < Hh).any() and (first == Hh).any()
            for misalign in ([False, True] if O % 4 == 0 else [False]):
                ret, costs = _run_kernel(pl, tr, act, misalign)
                _bits(ret, want_ret, 'returns (T %d, k0 %d, misalign %s)' % (T, k0, misalign))
                if variant == 'cem':
                    assert (costs == COST_GUARD).all()
                else:
                    _bits(costs, want_costs, 'cost bytes (T %d, k0 %d, misalign %s)' % (T, k0, misalign))
                    assert rows < 9 or (want_costs.any() and not want_costs.all())
        # the clip off too (returns reach -inf on the NaN row); the clock the setter left is (0, zeros)
        task = tk.tracking_task_for(O, A, Hh + 1, 0, False)
        pl.set_task(task)
        ret, _ = _run_kernel(pl, tr, act)
        _bits(ret, tracking_objective(tr, act, task, variant)[0], 'returns without a clip, at the reset clock')
        # k0 alone moves, the previous action stays
        pl.set_task_clock(0, prev)
        pl.set_task_clock(2)
        assert pl.task_clock[0] == 2 and np.array_equal(pl.task_clock[1], prev)
        ret, _ = _run_kernel(pl, tr, act)
        _bits(ret, tracking_objective(tr, act, task, variant, k0=2, prev_action=prev)[0], 'returns after k0 alone was set')
    finally:
        pl.close()


@pytest.mark.parametrize('shape', [tk.SHAPES[1], tk.SHAPES[3]], ids=lambda s: 'O%d_A%d_H%d_rows%d_P%d' % s)
def test_kernel_on_a_cost_handle_masks_nothing(shape):
    _torch()
    O, A, Hh, rows, Pp = shape
    T, k0 = Hh + 1, 3
    task = tk.tracking_task_for(O, A, T, 1, True)
    prev = tk.prev_action_for(A, 1)
    pl = CemPlanner(dataclasses.replace(tc.kernel_handle_config(O, A, Pp, 'cost'), task=task))
    try:
        pl.set_task_clock(k0, prev)
        tr, act = tc.random_case(O, A, Hh, rows, Pp, 1)
        tk.craft(tr, act, task, k0, prev)
        ret, costs = _run_kernel(pl, tr, act)
        want_ret, want_costs = tracking_objective(tr, act, task, 'cost', k0=k0, prev_action=prev)
        _bits(ret, want_ret)
        _bits(costs, want_costs)
        assert want_costs.sum() > tracking_objective(tr, act, task, 'safe', k0=k0, prev_action=prev)[1].sum()
    finally:
        pl.close()


@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_where_the_contracts_meet_the_kernel_is_the_quadratic_kernel(variant):
    """T = 1, ref[0] = g, no terminal weights, no action rate: cem_task_score_kernel's returns and cost bytes on a second handle, bit for
    bit, on every shape and whatever the clock says."""
    _torch()
    for (O, A, Hh, rows, Pp) in tk.SHAPES:
        quad = tc.task_for(O, A, 0, True)
        tb = quad.tables(O, A)
        trk = TrackingTask(reference=tb['g'][None], q=quad.q, c=quad.c, goal_mask=quad.goal_mask, lo=quad.lo, hi=quad.hi, rho=quad.rho,
                           goal_radius=quad.goal_radius, reward_goal=quad.reward_goal, reward_clip=quad.reward_clip)
        cfg = tc.kernel_handle_config(O, A, Pp, variant)
        a, b = CemPlanner(dataclasses.replace(cfg, task=quad)), CemPlanner(dataclasses.replace(cfg, task=trk))
        try:
            tr, act = tc.random_case(O, A, Hh, rows, Pp, 0)
            tc.craft(tr, quad)
            b.set_task_clock(5, tk.prev_action_for(A))
            ra, ca = _run_kernel(a, tr, act)
            rb, cb = _run_kernel(b, tr, act)
            _bits(rb, ra, 'returns, O %d' % O)
            _bits(cb, ca, 'cost bytes, O %d' % O)
            _bits(ra, task_objective(tr, act, quad, variant)[0])
        finally:
            a.close(); b.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# plans: N = 64, H = 10, P = 2, E = 2, two iterations
# ---------------------------------------------------------------------------------------------------------------------------------
_PROBLEM = []
T_PLAN = H + 4


def _problem():
    if not _PROBLEM:
        _PROBLEM.append(hp.make_problem(obs_dim=60, act_dim=2, E=E, n_layers=4, seed=77))
    return _PROBLEM[0]


def _configs(variant='cem', I=2, precision='fp32', **kw):
    pb = _problem()
    _, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=K, I=I, variant=variant, precision=precision, post=0.3, **kw)
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


def _calibrated_task(pl, pb):
    """A tracking task whose thresholds are taken from the handle's own first rollout, as tests/test_gpu_task_scorer.py's: the reference
    starts a little off the start state and drifts by a fixed step per row (the last row jumps), R2 is the median over the rows of the
    closest a row gets to its reference after t = 0, the box lies between the 10 % and 90 % quantiles of features 2 .. 9.  (Thresholds of
    the TEST's task, not bars: every check below is bit for bit against the mirror on the device's own trajectories.)"""
    O = pb['state'].shape[0]
    pl.set_task(QuadraticTask(q=1.0, g=pb['state']))
    per, _ = _run_all(pl, pb['state'], SEED, 900)
    tr = per[0]['traj'].astype(np.float64)
    rng = np.random.default_rng(3)
    sd = tr[:, H // 2].std(axis=0)
    ref = pb['state'].astype(np.float64) + np.arange(T_PLAN)[:, None] * (0.05 * sd * rng.choice([-1.0, 1.0], O))
    ref[:, :2] += sd[:2]
    ref[-1] += 0.5 * sd
    rows = ref[np.minimum(np.arange(H + 1), T_PLAN - 1)]
    nsum = ((tr[:, :H, :2] - rows[:H, :2]) ** 2).sum(axis=2)
    radius = float(np.sqrt(np.median(nsum[:, 1:].min(axis=1))))
    lo, hi, m = np.full(O, -np.inf, F), np.full(O, np.inf, F), np.zeros(O, F)
    lo[2:10] = np.quantile(tr[:, 1:, 2:10], 0.1, axis=(0, 1))
    hi[2:10] = np.quantile(tr[:, 1:, 2:10], 0.9, axis=(0, 1))
    m[:2] = 1.0
    q = rng.uniform(0.0, 1.0, O).astype(F)
    task = TrackingTask(reference=ref.astype(F), q=q, c=rng.normal(0, 0.01, O).astype(F), goal_mask=m, lo=lo, hi=hi, rho=[0.1, 0.2],
                        goal_radius=radius, reward_goal=0.05, terminal_weights=(4.0 * q).astype(F), action_rate=[0.3, 0.15])
    pl.set_task(task)
    return task


PREV = np.array([0.25, -0.5], F)


def _planner(variant='cem', **kw):
    _torch()
    pb, pcfg = _configs(variant=variant, **kw)
    pl = hp.make_planner(pb, pcfg)
    return pb, pcfg, pl, _calibrated_task(pl, pb)


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


def _check_iteration(rec, task, variant, pcfg, k0, prev, n=N, what=''):
    """One iteration's returns, cost bytes and scores against the mirror on the trajectories and the sample the device itself held."""
    traj, act = rec['traj'][:P * n], rec['actions'][:n]
    ret, costs = tracking_objective(traj, act, task, variant, k0=k0, prev_action=prev)
    _bits(rec['returns'][:P * n], ret, '%s: returns' % what)
    if variant != 'cem':
        _bits(rec['costs'][:H * P * n].reshape(H, P * n), costs, '%s: cost bytes' % what)
    _bits(rec['scores'][:n], _restated_scores(variant, ret, costs, pcfg, n), '%s: scores' % what)
    return ret, costs


@pytest.mark.parametrize('variant', ['cem', 'safe', 'cost'])
def test_scores_of_two_iterations_and_the_three_plan_forms(variant):
    pb, pcfg, pl, task = _planner(variant=variant)
    others = []
    k0 = 2
    try:
        pl.set_task_clock(k0, PREV)
        per, (a, s, iters) = _run_all(pl, pb['state'], SEED, 0)
        seen_done = seen_cost = False
        for it in range(2):
            ret, costs = _check_iteration(per[it], task, variant, pcfg, k0, PREV, what='%s iteration %d' % (variant, it))
            first = tracking_objective(per[it]['traj'], per[it]['actions'], task, variant, k0=k0, prev_action=PREV, return_done=True)[2]
            seen_done |= bool((first < H).any() and (first == H).any())
            seen_cost |= costs is not None and bool(costs.any() and not costs.all())
            # the clock reached the plan: the mirror at the reset clock says something else
            assert not np.array_equal(ret, tracking_objective(per[it]['traj'], per[it]['actions'], task, variant)[0])
        assert seen_done or variant == 'cost'
        assert seen_cost or variant == 'cem'
        assert not np.array_equal(per[0]['scores'], per[1]['scores'])
        # eager and graph plans on handles of their own, Philox noise: the same action, score and iteration count
        for use_graph in (False, True):
            _, cfg2 = _configs(variant=variant, use_graph=use_graph)
            p2 = hp.make_planner(pb, dataclasses.replace(cfg2, task=task))
            others.append(p2)
            p2.set_task_clock(k0, PREV)
            for _ in range(2):                                     # (the second graph plan replays the captured one)
                a2, s2, i2 = p2.plan(pb['state'], seed=SEED, call=0)
                _bits(a2, a, 'action, use_graph %s' % use_graph)
                assert F(s2).view(U) == F(s).view(U) and i2 == iters
            assert p2.graph_status() == ('graph' if use_graph else 'eager')
            assert p2.rollout_path() == 'generic' and p2.iteration_plan(0)['rollout_path'] == 'generic'
    finally:
        for p in [pl] + others:
            p.close()


def test_the_clock_is_not_baked_into_the_graph():
    """Handle X follows R, handle Y follows R[3:].  X plans once as a graph at k0 = 0; then X's clock is set to (3, a) and Y's to (0, a):
    both now compare every state with the same rows, and the same seed and call give the same result-block words, action and returns —
    X through the graph it captured before the clock moved, with the node count it had."""
    _torch()
    pb, pcfg = _configs(use_graph=True)
    probe = hp.make_planner(pb, _configs()[1])
    try:
        task = _calibrated_task(probe, pb)
    finally:
        probe.close()
    x = hp.make_planner(pb, dataclasses.replace(pcfg, task=task))
    y = hp.make_planner(pb, dataclasses.replace(pcfg, task=dataclasses.replace(task, reference=np.asarray(task.reference)[3:].copy())))
    try:
        x.plan(pb['state'], seed=SEED, call=0)
        assert x.graph_status() == 'graph'
        nodes = x.graph_nodes()
        assert nodes > 0
        x.plan(pb['state'], seed=SEED, call=1)
        at_zero = _np(x.returns())
        x.set_task_clock(3, PREV)
        y.set_task_clock(0, PREV)
        ax, sx, ix = x.plan(pb['state'], seed=SEED, call=1)
        ay, sy, iy = y.plan(pb['state'], seed=SEED, call=1)
        _bits(ax, ay, 'actions')
        _bits(_np(x.returns()), _np(y.returns()), 'returns')
        _bits(_np(x.result_block())[:36], _np(y.result_block())[:36], 'result block')
        assert F(sx).view(U) == F(sy).view(U) and ix == iy
        assert x.graph_status() == 'graph' and x.graph_nodes() == nodes
        assert not np.array_equal(_np(x.returns()), at_zero)       # (and the clock is read: the same call at k0 = 0 returned something else)
        # what the graph scored is the mirror's at the clock it was given after the capture
        ret, _ = tracking_objective(_np(x.task_trajectories()), _np(x.actions()), task, 'cem', k0=3, prev_action=PREV)
        _bits(_np(x.returns()).reshape(-1), ret, 'the last iteration of the replayed graph')
    finally:
        x.close(); y.close()


def test_with_plan_readout():
    pb, pcfg, pl, task = _planner(I=1)
    try:
        pl.set_plan_readout(True)
        pl.set_task_clock(1, PREV)
        a, s, _ = pl.plan(pb['state'], seed=SEED, call=0)
        ro = pl.plan_readout()
        ret, _ = tracking_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'cem', k0=1, prev_action=PREV)
        assert ro.iteration == 0 and 0 <= ro.candidate < N
        _bits(ro.particle_returns, ret.reshape(P, N)[:, ro.candidate], 'particle returns of the winner')
        _bits(ro.sequence[0], a)
        assert F(ro.score).view(U) == F(cc.mean_returns(ret.reshape(P, N))[ro.candidate]).view(U) == F(s).view(U)
    finally:
        pl.close()


def test_with_a_population_schedule():
    pb, pcfg, pl, task = _planner()
    n1 = 40
    try:
        pl.set_population_schedule([N, n1])
        pl.set_task_clock(4, PREV)
        assert pl.iteration_plan(1)['n_samples'] == n1 and pl.iteration_plan(1)['rollout_path'] == 'generic'
        pl.plan_begin(pb['state'], SEED, 0)
        for it, n in ((0, N), (1, n1)):
            pl.plan_rollout(it)
            rec = dict(traj=_np(pl.task_trajectories()), actions=_np(pl.actions()), scores=_np(pl.scores_local()),
                       returns=_np(pl.returns()).reshape(-1), costs=None)
            _check_iteration(rec, task, 'cem', pcfg, 4, PREV, n=n, what='iteration %d' % it)
            pl.plan_select(it)
        _, score, iters = pl.plan_end()
        assert np.isfinite(score) and iters == 2
    finally:
        pl.close()


def test_with_bf16():
    pb, pcfg, pl, task = _planner(variant='safe', precision='bf16')
    try:
        pl.set_task_clock(2, PREV)
        per, _ = _run_all(pl, pb['state'], SEED, 0)
        for it in range(2):
            _check_iteration(per[it], task, 'safe', pcfg, 2, PREV, what='bf16 iteration %d' % it)
    finally:
        pl.close()


@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_set_then_clear_is_a_handle_that_never_had_a_task(variant):
    _torch()
    pb, pcfg = _configs(variant=variant, use_graph=True)
    never, cleared = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    try:
        cleared.set_task(tk.tracking_task_for(60, 2, H + 1))
        cleared.set_task_clock(1, PREV)
        on_plan = cleared.iteration_plan(0)
        cleared.plan(pb['state'], seed=SEED, call=0)
        assert cleared.rollout_path() == 'generic'
        cleared.set_task(None)
        assert cleared.task is None and cleared.task_clock is None
        assert cleared.rollout_path() == never.rollout_path()
        assert [cleared.iteration_plan(i) for i in range(2)] == [never.iteration_plan(i) for i in range(2)]
        assert on_plan['launches'] > never.iteration_plan(0)['launches']
        for call in range(2):
            a, s, i = never.plan(pb['state'], seed=SEED, call=call)
            a2, s2, i2 = cleared.plan(pb['state'], seed=SEED, call=call)
            _bits(a2, a)
            assert F(s2).view(U) == F(s).view(U) and i2 == i
        assert cleared.graph_status() == never.graph_status() == 'graph' and cleared.graph_nodes() == never.graph_nodes() > 0
        _bits(_np(cleared.result_block())[:36], _np(never.result_block())[:36])
        for call in (cleared.task_trajectories, lambda: cleared.set_task_clock(0)):
            with pytest.raises(_capi.CemError) as e:
                call()
            assert e.value.status == STATE
    finally:
        never.close(); cleared.close()


def test_refusals():
    _torch()
    pb, pcfg = _configs()
    task = tk.tracking_task_for(60, 2, H + 1)
    pl = hp.make_planner(pb, pcfg)
    fp = C.POINTER(C.c_float)
    try:
        before = pl.iteration_plan(0)
        # a clock call without a tracking task: none at all, then a quadratic one
        for quad in (None, tc.task_for(60, 2)):
            pl.set_task(quad)
            with pytest.raises(_capi.CemError) as e:
                pl.set_task_clock(0)
            assert e.value.status == STATE
        pl.set_task(None)
        ref = np.asarray(task.reference, F)
        nan_ref = ref.copy()
        nan_ref[H, 59] = np.nan
        bad = [dataclasses.replace(task, reference=nan_ref), dataclasses.replace(task, terminal_weights=np.full(60, np.inf, F)),
               dataclasses.replace(task, action_rate=[np.nan, 0.0]), dataclasses.replace(task, q=np.full(60, np.nan, F)),
               dataclasses.replace(task, lo=1.0, hi=0.5)]
        for b in bad:
            with pytest.raises(_capi.CemError) as e:
                pl.set_task(b)
            assert e.value.status == INVALID_ARG
        # through the C structs: base.g not NULL, another base kind, ref_steps 0 and above the cap, no reference
        g = np.zeros(60, F)
        big = np.zeros((_capi.CEM_TASK_REF_MAX_STEPS + 1, 60), F)
        quad = lambda **kw: _capi.CemTask(kind=_capi.CEM_TASK_QUADRATIC, **kw)
        trk = lambda a, n: _capi.CemTaskTracking(ref=a.ctypes.data_as(fp) if a is not None else None, ref_steps=n)
        for base, t in ((quad(g=g.ctypes.data_as(fp)), trk(ref, H + 1)), (_capi.CemTask(kind=_capi.CEM_TASK_TRACKING), trk(ref, H + 1)),
                        (_capi.CemTask(kind=_capi.CEM_TASK_SAFETY_GYM), trk(ref, H + 1)), (quad(), trk(ref, 0)), (quad(), trk(ref, -1)),
                        (quad(), trk(big, _capi.CEM_TASK_REF_MAX_STEPS + 1)), (quad(), trk(None, 1))):
            assert pl.lib.cem_planner_set_task_tracking(pl.h, C.byref(base), C.byref(t)) == INVALID_ARG
        # cem_planner_set_task itself accepts kinds 0 and 1 only
        assert pl.lib.cem_planner_set_task(pl.h, C.byref(_capi.CemTask(kind=_capi.CEM_TASK_TRACKING))) == INVALID_ARG
        assert pl.iteration_plan(0) == before and pl.task is None
        # the cap itself is served
        top = trk(big, _capi.CEM_TASK_REF_MAX_STEPS)
        assert pl.lib.cem_planner_set_task_tracking(pl.h, C.byref(quad()), C.byref(top)) == 0
        # the clock's own refusals; inside a stepwise plan both calls are refused
        pl.set_task(task)
        for k0, a in ((-1, None), (0, [np.nan, 0.0]), (0, [0.0, np.inf])):
            with pytest.raises(_capi.CemError) as e:
                pl.set_task_clock(k0, a)
            assert e.value.status == INVALID_ARG
        assert pl.task_clock[0] == 0 and not pl.task_clock[1].any()
        pl.plan_begin(pb['state'], SEED, 0)
        for call in (lambda: pl.set_task(task), lambda: pl.set_task_clock(1)):
            with pytest.raises(_capi.CemError) as e:
                call()
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
    finally:
        bp.close()
    _, cfg_w = _configs(world_size=2)
    pw = CemPlanner(cfg_w)
    try:
        with pytest.raises(_capi.CemError) as e:
            pw.set_task(task)
        assert e.value.status == UNSUPPORTED
    finally:
        pw.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# the policy: its clock, and a closed loop that follows a sine
# ---------------------------------------------------------------------------------------------------------------------------------
def _integrator_policy(task, cls=None, **kw):
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    c = tk.TRACK
    box = lambda lo, hi: types.SimpleNamespace(low=np.asarray(lo, F), high=np.asarray(hi, F), shape=(len(lo),))
    obs_space, act_space = box([-10.0, -10.0], [10.0, 10.0]), box([-1.0], [1.0])
    model = TransitionModel('mlp_ensemble', obs_space, act_space, scale_features=False, sampling_propagation=False, ensemble_size=c['E'],
                            mlp_params=dict(n_layers=2, units=tc.UNITS, activation='tf.nn.relu', dropout_rate=0.0))
    model.model.set_weights(tc.integrator_weights(c['E']))
    env = types.SimpleNamespace(action_space=act_space, observation_space=obs_space)
    return (cls or CemMpc)(model=model, environment=env, horizon=c['H'], iterations=c['I'], smoothing=0.0, n_samples=c['N'], n_elite=c['k'],
                           particles=c['P'], stddev_threshold=-1.0, noise_stddev=0.0, seed=SEED, task=task, **kw)


def test_the_policy_keeps_the_clock():
    """Three decisions, reset(), one more: the handle's clock reads (0, 0), (1, a_0), (2, a_1), then (0, 0) again."""
    _torch()
    pol = _integrator_policy(tk.sine_task(action_rate=0.05))
    s = np.array([0.0, 0.0], F)
    actions = []
    for k in range(3):
        a = pol.generate_action(s)
        k0, prev = pol._planner.task_clock
        assert k0 == k and np.array_equal(prev, actions[-1] if actions else np.zeros(1, F)), (k, k0, prev)
        actions.append(np.array(a, F))
        s = tc.integrator_step(s, a[0])
    assert any(a.any() for a in actions)
    pol.reset()
    pol.generate_action(s)
    k0, prev = pol._planner.task_clock
    assert k0 == 0 and not prev.any()
    with pytest.raises(ValueError, match='batch handle'):
        pol.generate_actions(np.zeros((2, 2), F))


def test_the_policy_counts_the_decisions_between_two_plans():
    _torch()
    pol = _integrator_policy(tk.sine_task(), replan_every=2)
    s = np.array([0.0, 0.0], F)
    seen = []
    for k in range(4):
        a = pol.generate_action(s)
        seen.append((pol._planner.task_clock[0], np.array(pol._planner.task_clock[1], F), np.array(a, F)))
        s = tc.integrator_step(s, a[0])
    # plans at decisions 0 and 2: the clock of the second is (2, the action FOLLOWED at decision 1)
    assert [k for k, _, _ in seen] == [0, 0, 2, 2]
    _bits(seen[2][1], seen[1][2])


def test_closed_loop_follows_a_sine():
    """CemMpc(task=TrackingTask(...)) drives task_cases' double integrator (the ensemble set by hand to its exact dynamics, model noise
    off) from rest at the origin along pos = 0.3 sin(2 pi k / 40) with the matching velocity row: N = 64, H = 10, I = 3, k = 8, P = 2,
    q = (1, 0.1), qT = 4 q, rho = 0.01, kappa = 0, 80 decisions.  The yardstick is a NumPy CEM on the same model scored by
    planner.tracking_objective (tracking_cases.reference_closed_loop), seeds 0 .. 4, measured on the CPU: its worst RMS position error
    over decisions 40 .. 79 is 0.0207 (not tracking at all: 0.212), its largest |vel| 0.530.  The policy's RMS error stays within
    2 x 0.0207 and its executed trajectory inside the velocity box of 1.0."""
    _torch()
    c = tk.TRACK
    task = tk.sine_task()
    pol = _integrator_policy(task)
    s = np.array([0.0, 0.0], F)
    states, vmax = [], 0.0
    for step in range(c['steps']):
        states.append(s.copy())
        a = pol.generate_action(s)
        if step == 7:
            pl = pol._planner
            assert isinstance(pl.task, TrackingTask) and pl.rollout_path() == 'generic' and pl.task_clock[0] == 7
            # what the plan scored last is the mirror's at the policy's clock
            ret, _ = tracking_objective(_np(pl.task_trajectories()), _np(pl.actions()), task, 'cem', k0=7, prev_action=pl.task_clock[1])
            _bits(_np(pl.returns()).reshape(-1), ret, 'returns of decision 7')
        s = tc.integrator_step(s, a[0])
        vmax = max(vmax, abs(float(s[1])))
    rms = tk.rms_position_error(np.array(states))
    print('sine tracking: RMS position error %.4f (reference worst %.4f, untracked %.3f), largest |vel| %.3f'
          % (rms, tk.REFERENCE_WORST_RMS, tk.UNTRACKED_RMS, vmax))
    assert rms <= 2 * tk.REFERENCE_WORST_RMS, rms
    assert vmax <= tc.VEL_BOX, vmax
