"""The cost-minimising objective on the device (CEM_VARIANT_COST; SafeCemMpc.optimize_for_safety / compute_mean_costs, reference
simba/policies/safe_cem_mpc.py:40-74,98-108) against its NumPy restatement (tests/cost_cases.py).

What is exact and what is not: the new reduce kernel is integer counting and one division, so its scores equal the restatement on the
device's own cost bytes bit for bit; the bytes themselves come from the rollout's fp32 states, so against the fp64 oracle a byte may
differ where a closest distance lies within the trajectory tolerance of tests/test_gpu_parity.py (5e-6) of its cost size.  Selection is
compared on the device's own scores (ties are massive: many candidates cost nothing), mu / sigma at that file's tolerance for the
one-workgroup select."""
import dataclasses

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import cost_cases as cc
from tests import helpers as hp

pytestmark = pytest.mark.gpu

TRAJ_ATOL = 5e-6                 # tests/test_gpu_parity.py ATOL: |gpu - oracle64| of unfold_sequences trajectories
O, A = 60, 2


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _first_rollout(pl, pb, ea, em):
    """begin + rollout(0) -> (cost bytes [H, P, N], scores [N], actions [N, H, A]) as the device left them."""
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    pl.plan_rollout(0)
    return pl.costs().cpu().numpy().copy(), pl.scores_local().cpu().numpy().copy(), pl.actions().cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------- 1: the reduce kernel, bit for bit
REDUCE_SHAPES = {                # N, P, H, E, problem
    'n70_h4': (70, 5, 4, 5, dict()),                                   # N not a multiple of 64, H < 16, H P = 20: four waves idle past the first row each
    'n64_h16': (64, 5, 16, 5, dict()),
    'n200_h17': (200, 5, 17, 5, dict()),                               # several blocks, H P = 85 not a multiple of the 16 waves
    'p45_h8': (150, 45, 8, 15, dict()),                                # the shipped particles: H P = 360, two trips of 16 loads
    'p3_h33': (96, 3, 33, 3, dict()),
    'four_kinds_sum': (70, 5, 4, 5, dict(kinds=(0, 1, 2, 3), indicator=False)),     # counts above 1 per step
}


def _check_reduce(pb, pcfg, N, P, H, seed=8):
    pl = hp.make_planner(pb, pcfg)
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=seed)
    costs, scores, _ = _first_rollout(pl, pb, ea, em)
    want = cc.scores_from_bytes(costs, P, N)
    print('cost bytes: mean %.3f max %d; scores %.3f .. %.3f, %d distinct' % (costs.mean(), costs.max(), scores.min(), scores.max(), np.unique(scores).size))
    np.testing.assert_array_equal(scores, want)
    assert costs.min() == 0 and costs.max() >= 1 and np.unique(scores).size > 1, 'the case should see candidates of different cost'
    pl.close()
    return costs


@pytest.mark.parametrize('case', list(REDUCE_SHAPES))
def test_reduce_kernel_equals_the_restatement_on_the_devices_bytes(case):
    _torch()
    N, P, H, E, prob = REDUCE_SHAPES[case]
    pb = cc.problem(E=E, **prob)
    _, pcfg = cc.configs(pb, N=N, H=H, P=P, E=E, k=max(2, N // 10), I=1)
    costs = _check_reduce(pb, pcfg, N, P, H)
    if case == 'four_kinds_sum':
        assert 1 < costs.max() <= 4, costs.max()


@pytest.mark.parametrize('how', ['bf16x3', 'tanh256'])
def test_reduce_kernel_behind_the_other_rollout_kernels(how):
    """All three rollout kernels store their cost bytes through the one bookkeeping macro: the split-product and the generic kernel too."""
    _torch()
    N, P, H, E = 70, 5, 4, 5
    pb = cc.problem(E=E) if how == 'bf16x3' else cc.problem(E=E, units=256, activation='tanh')
    _, pcfg = cc.configs(pb, N=N, H=H, P=P, E=E, k=7, I=1, **(dict(precision='bf16x3') if how == 'bf16x3' else {}))
    assert (pcfg.precision, pcfg.units, pcfg.activation) == (('bf16x3', 128, 'relu') if how == 'bf16x3' else ('fp32', 256, 'tanh'))
    _check_reduce(pb, pcfg, N, P, H)


# ------------------------------------------------------------------------------------------------- 2: un-masked
def test_costs_are_not_masked_by_done():
    """A start state inside the goal radius with a hazard inside its size: the safe variant's done mask zeroes every cost byte from step
    0 on, a cost handle on the same inputs stores the costs themselves."""
    _torch()
    N, P, H, E = 70, 5, 6, 5
    pb = cc.problem(E=E, size_frac=1.5, near_goal=True)
    sp = pb['scorer']
    assert o.goal_distance_metric(pb['state'][None], sp)[0] <= np.float32(sp.goal_size * 0.8) and o.cost(pb['state'][None], sp)[0] == 1
    ocfg, pcost = cc.configs(pb, N=N, H=H, P=P, E=E, k=7, I=1)
    psafe = dataclasses.replace(pcost, variant='safe')
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=12)
    pl_c, pl_s = hp.make_planner(pb, pcost), hp.make_planner(pb, psafe)
    costs_c, scores_c, actions = _first_rollout(pl_c, pb, ea, em)
    costs_s, _, _ = _first_rollout(pl_s, pb, ea, em)
    assert costs_s.max() == 0                                           # every row is done at step 0
    assert (costs_c[0] == 1).all() and (costs_c > costs_s).any(axis=(1, 2)).all()      # step 0 is s_0's cost; every step has rows that cost
    np.testing.assert_array_equal(scores_c, cc.scores_from_bytes(costs_c, P, N))
    # ... and the restatement on the oracle's fp32 trajectories, where no cost comparison is within the trajectory tolerance of flipping
    s0 = np.broadcast_to(pb['state'], (P * N, O)).copy()
    traj = o.unfold_sequences(s0.astype(np.float64), np.tile(actions, (P, 1, 1)).astype(np.float64), o.cast_weights(pb['weights'], np.float64),
                              o.member_of_rows(P * N, E), pb['inputs_min'], pb['inputs_max'], em[0].astype(np.float64))
    clear = (cc.cost_margins(traj, sp) > TRAJ_ATOL).reshape(H, P, N).all(axis=(0, 1))
    assert clear.mean() >= 0.9
    np.testing.assert_array_equal(scores_c[clear], cc.mean_cost_scores(traj, P, N, sp).astype(np.float32)[clear])
    pl_c.close(); pl_s.close()


# ------------------------------------------------------------------------------------------------- 3: the bytes against the oracle
BYTES_SEED = 8


def test_cost_bytes_against_the_fp64_oracle():
    """Bytes from oracle.unfold_sequences in fp64 + oracle.cost.  A device byte may differ only where the fp64 shadow's
    |closest_distance - cost_size| of some kind is below 5e-6, and at most 1 % of the bytes may lie that close.
    Noise seed 8 on cost_cases.problem(size_frac=0.99) (sizes 1 % inside the start state's distances: at 1.0 every row's step 0 sits
    ON its size), N = 200, P = 5, H = 17, chosen on the CPU with the oracle alone (sampled actions, unfold_sequences in fp32 and in
    fp64, oracle.cost on both): of the 17 000 bytes, 0 lie within 5e-6 of a size in the fp64 shadow (the closest is 9.5e-5 away) and
    the oracle's fp32 bytes differ from its fp64 bytes at 0 of them; the mean cost is 0.727.  (Seed 9: 1 byte that close, 0 differ.)"""
    _torch()
    N, P, H, E = 200, 5, 17, 5
    pb = cc.problem(E=E, size_frac=0.99)
    sp = pb['scorer']
    _, pcfg = cc.configs(pb, N=N, H=H, P=P, E=E, k=20, I=1)
    pl = hp.make_planner(pb, pcfg)
    ea, em, _ = hp.noise(1, N, H, A, P, O, seed=BYTES_SEED)
    costs, _, actions = _first_rollout(pl, pb, ea, em)
    s0 = np.broadcast_to(pb['state'], (P * N, O)).astype(np.float64)
    traj = o.unfold_sequences(s0, np.tile(actions, (P, 1, 1)).astype(np.float64), o.cast_weights(pb['weights'], np.float64),
                              o.member_of_rows(P * N, E), pb['inputs_min'], pb['inputs_max'], em[0].astype(np.float64))
    want = cc.cost_bytes(traj, sp).reshape(H, P, N)
    near = (cc.cost_margins(traj, sp) < TRAJ_ATOL).reshape(H, P, N)
    differ = costs != want
    print('bytes: %d of %d differ from the fp64 oracle, %d within %.0e of a size; mean cost %.3f' % (differ.sum(), differ.size, near.sum(), TRAJ_ATOL, want.mean()))
    assert near.mean() <= 0.01
    assert not (differ & ~near).any(), 'bytes differ where no distance is near its size: %s' % (np.argwhere(differ & ~near)[:5],)
    assert 0.02 < want.mean() < 0.98
    pl.close()


# ------------------------------------------------------------------------------------------------- 4: iterations, flip-proof
def test_iterations_select_on_the_devices_own_scores():
    """Three iterations through the stepwise calls; after every rollout the oracle's select_and_refit runs on the DEVICE's scores and
    actions, so no cost comparison can flip between the two sides.  Elite set exact (ties to the lowest index), best action and score
    exact, mu / sigma at tests/test_gpu_parity.py's tolerance for the one-workgroup select."""
    torch = _torch()
    N, P, H, E, k, I = 200, 5, 8, 5, 20, 3
    pb = cc.problem(E=E)
    ocfg, pcfg = cc.configs(pb, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1)
    pl = hp.make_planner(pb, pcfg)
    assert pl.select_mode() == 1
    ea, em, _ = hp.noise(I, N, H, A, P, O, seed=9)
    pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
    best, best_score, tied_past_k = np.zeros(A, np.float32), np.float32(-np.inf), 0
    for it in range(I):
        pl.plan_rollout(it)
        scores, actions, ms0 = pl.scores_local().cpu().numpy().copy(), pl.actions().cpu().numpy().copy(), pl.mu_sigma().cpu().numpy().copy()
        np.testing.assert_array_equal(scores, cc.scores_from_bytes(pl.costs().cpu().numpy(), P, N))
        mu, sigma, best, best_score, elite, _ = o.select_and_refit(scores, actions, ms0[0], ms0[1], best, best_score, ocfg)
        kth = np.sort(scores)[::-1][k - 1]
        tied_past_k = max(tied_past_k, int((scores == kth).sum()) if (scores >= kth).sum() > k else 0)
        pl.plan_select(it)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(np.sort(pl.elite_idx().cpu().numpy()), elite)
        ms1 = pl.mu_sigma().cpu().numpy()
        np.testing.assert_allclose(ms1[0], mu, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(ms1[1], sigma, rtol=1e-5, atol=1e-7)
    a, s, n_it = pl.plan_end(eps_out=np.zeros(A, np.float32))
    np.testing.assert_array_equal(a, best)
    assert s == best_score and n_it == I
    assert tied_past_k > 0, 'no iteration had more candidates tied at the k-th score than fit the elite set: the tie rule was not exercised'
    pl.close()


# ------------------------------------------------------------------------------------------------- 5: the whole plan
def test_whole_plan_graph_eager_and_stepwise_agree():
    torch = _torch()
    N, P, H, E, k, I = 200, 5, 8, 5, 20, 4
    pb = cc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1, noise=0.03)
    pg, pe, ps = (hp.make_planner(pb, cc.configs(pb, use_graph=g, **kw)[1]) for g in (True, False, False))
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
        assert sg == se == s2 <= 0 and ig == ie == i2 == I
        for view in ('mu_sigma', 'elite_idx', 'scores_local', 'actions', 'costs'):
            assert torch.equal(getattr(pg, view)(), getattr(ps, view)()) and torch.equal(getattr(pe, view)(), getattr(ps, view)()), (view, call)
    assert (pg.graph_status(), pe.graph_status()) == ('graph', 'eager')
    for p in (pg, pe, ps):
        p.close()


def test_early_stop_returns_the_restated_loops_iteration_count():
    """stddev_threshold 0.25: the stepwise plan is stopped where the restated loop, run on the device's scores, stops; the whole plan
    (graph) returns the same count, action and score."""
    torch = _torch()
    N, P, H, E, k, I = 200, 5, 8, 5, 5, 10                 # (5 elites of 200: on the CPU, with other noise, the restated loop stops after 4 - 5 iterations)
    pb = cc.problem(E=E)
    kw = dict(N=N, H=H, P=P, E=E, k=k, I=I, thr=0.25)
    ocfg, pcfg = cc.configs(pb, **kw)
    ps, pg = hp.make_planner(pb, pcfg), hp.make_planner(pb, cc.configs(pb, use_graph=True, **kw)[1])
    ps.plan_begin(pb['state'], seed=5, call=2)
    best, best_score, iters = np.zeros(A, np.float32), np.float32(-np.inf), 0
    for it in range(I):                                     # the loop of cost_cases.plan_cost, scores / actions / mu / sigma the device's
        ps.plan_rollout(it)
        scores, actions, ms0 = ps.scores_local().cpu().numpy().copy(), ps.actions().cpu().numpy().copy(), ps.mu_sigma().cpu().numpy().copy()
        _, sigma, best, best_score, _, stop = o.select_and_refit(scores, actions, ms0[0], ms0[1], best, best_score, ocfg)
        ps.plan_select(it)
        iters += 1
        print('iteration %d: mean sigma %.4f (restated), %.4f (device)' % (it, sigma.mean(), ps.mu_sigma().cpu().numpy()[1].mean()))
        if stop:
            break
    a2, s2, i2 = ps.plan_end()
    assert i2 == iters and 1 <= iters < I, (i2, iters)
    np.testing.assert_array_equal(a2, best)
    assert s2 == best_score
    ag, sg, ig = pg.plan(pb['state'], seed=5, call=2)
    assert ig == iters and sg == s2
    np.testing.assert_array_equal(ag, a2)
    ps.close(); pg.close()


# ------------------------------------------------------------------------------------------------- 6: batch handles
def test_batch_problems_equal_their_single_cost_plans():
    torch = _torch()
    from ethz_safe_learning_amd import BatchCemPlanner
    N, P, H, E, k, I, mb, n = 200, 5, 8, 5, 20, 3, 4, 3
    pb = cc.problem(E=E)
    _, pcfg = cc.configs(pb, N=N, H=H, P=P, E=E, k=k, I=I, smoothing=0.1, noise=0.02, use_graph=True)
    single = hp.make_planner(pb, pcfg)
    batch = BatchCemPlanner(pcfg, mb)
    batch.set_weights(pb['weights']); batch.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    rng = np.random.default_rng(4)
    states = np.repeat(pb['state'][None], n, 0)
    states[1:] += rng.normal(0, 0.05, states[1:].shape).astype(np.float32)
    calls = np.array([7, 1 << 33, 9], np.uint64)
    lay = batch.layout

    def slices():
        batch.synchronize()
        v = dict(scores=batch._view(lay.scores_local, mb * N, torch.float32).view(mb, N), elite=batch._view(lay.elite_idx, mb * k, torch.int32).view(mb, k),
                 actions=batch._view(lay.actions, mb * N * H * A, torch.float32).view(mb, N, H, A), costs=batch._view(lay.costs, mb * H * P * N, torch.uint8).view(mb, H, P, N),
                 musig=batch._view(lay.mu_sigma, mb * 2 * H * A, torch.float32).view(mb, 2, H, A))
        return {key: t.cpu().numpy().copy() for key, t in v.items()}
    before = slices()
    acts, scores, iters = batch.plan_batch(states, seed=3, calls=calls)
    after = slices()
    assert batch.graph_status() == 'graph' and batch.launches_per_iteration() == 3
    for b in range(n):
        a1, s1, i1 = single.plan(states[b], seed=3, call=int(calls[b]))
        np.testing.assert_array_equal(acts[b], a1)
        assert scores[b] == s1 and iters[b] == i1
        np.testing.assert_array_equal(after['scores'][b], single.scores_local().cpu().numpy())
        np.testing.assert_array_equal(after['costs'][b], single.costs().cpu().numpy())
        np.testing.assert_array_equal(after['scores'][b], cc.scores_from_bytes(after['costs'][b], P, N))
        np.testing.assert_array_equal(after['musig'][b], single.mu_sigma().cpu().numpy())
        np.testing.assert_array_equal(np.sort(after['elite'][b]), np.sort(single.elite_idx().cpu().numpy()))
    for key in ('scores', 'elite', 'actions', 'costs'):                  # the fourth problem was staged as stopped: its slices are as they were
        np.testing.assert_array_equal(after[key][n:], before[key][n:], err_msg=key)
    single.close(); batch.close()


# ------------------------------------------------------------------------------------------------- 7: the op and the policy
def test_compute_mean_costs_is_the_restatement_on_an_unfolded_tensor():
    torch = _torch()
    from tests.test_simba_api import make_agent_parts, trained_like
    env, model, pol = make_agent_parts('safe_cem_mpc', seed=3)
    trained_like(model, np.random.default_rng(0))
    P, n, H = pol.particles, 30, 5
    rng = np.random.default_rng(1)
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    s0 = np.repeat(PointGoalEnv(n_hazards=8, seed=2, config=dict(constrain_hazards=True)).reset()[None].astype(np.float32), P * n, 0)
    acts = np.tile(rng.uniform(-1, 1, (n, H, pol.action_space.shape[0])).astype(np.float32), (P, 1, 1))
    traj = model.unfold_sequences(s0, acts)
    traj_t = traj if torch.is_tensor(traj) else torch.as_tensor(traj, device='cuda:0')
    traj_np = traj_t.cpu().numpy()
    sp = env._scorer.to_scorer_config()
    osp = o.ScorerParams(goal_slice=tuple(sp.goal_slice), observe_goal_lidar=sp.observe_goal_lidar, lidar_max_dist=sp.lidar_max_dist, goal_size=sp.goal_size,
                         reward_distance=sp.reward_distance, reward_goal=sp.reward_goal, reward_clip=sp.reward_clip,
                         constrain_indicator=sp.constrain_indicator, cost_kinds=list(sp.cost_kinds))
    want = -cc.mean_cost_scores(traj_np, P, n, osp)
    got_np = pol.compute_mean_costs(traj_np, acts)
    got_t = pol.compute_mean_costs(traj_t)
    assert isinstance(got_np, np.ndarray) and got_np.dtype == np.float32 and torch.is_tensor(got_t) and got_t.is_cuda
    np.testing.assert_array_equal(got_np, want)
    np.testing.assert_array_equal(got_t.cpu().numpy(), want)
    assert (got_np >= 0).all()
    # the safe objective on the same tensor is another function (and the class's own objective handle is untouched by the cost one)
    assert pol.compute_objective(traj_np).shape == (n,)


def _policy(recover_below='absent', seed=3):
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    env, model, pol = make_agent_parts('safe_cem_mpc', seed=seed)
    trained_like(model, np.random.default_rng(0))
    if recover_below != 'absent':
        pol = SafeCemMpc(model=model, environment=env, recover_below=recover_below, **dict(POLICIES_YAML['safe_cem_mpc']))
    return env, model, pol


def _states(n):
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    return np.stack([PointGoalEnv(seed=s).reset() for s in range(n)]).astype(np.float32)


def test_optimize_for_safety_returns_an_action_inside_the_box():
    _torch()
    env, model, pol = _policy()
    pol.noise_stddev = 0.0
    a = pol.optimize_for_safety(_states(1)[0])
    assert a.shape == (pol.action_space.shape[0],) and a.dtype == np.float32
    assert (a >= pol.action_space.low).all() and (a <= pol.action_space.high).all()
    assert pol.last_safety_score <= 0 and pol._cost_planner.cfg.variant == 'cost'
    assert pol._cost_planner.launches_per_iteration() == 3                       # 8: rollout, cost reduce, select at the shipped shape
    b = pol.optimize_for_safety(_states(1)[0], call=0)
    np.testing.assert_array_equal(a, b)                                        # (seed, call) reproduces
    pol.optimize_for_safety(_states(1)[0], call=1)
    assert pol._cost_planner.graph_status() == 'graph'


def test_recovery_is_opt_in_and_replaces_the_plan_below_the_threshold():
    _torch()
    st = _states(1)[0]
    _, _, plain = _policy()
    _, _, off = _policy(recover_below=None)
    _, _, always = _policy(recover_below=float('inf'))
    for p in (plain, off, always):
        p.build()
        p._planner._call = 50                                                  # (policies of one shape share the cached handle)
        p.got = p.generate_action(st)
    np.testing.assert_array_equal(off.got, plain.got)                          # None: bit for bit the policy without the key
    assert off._cost_planner is None and off.last_recovered is None and not off._cost_batch_planners
    assert always.last_recovered is True
    np.testing.assert_array_equal(always.got, always.optimize_for_safety(st, call=50))
    assert not np.array_equal(always.got, plain.got)
    _, _, never = _policy(recover_below=-1e9)
    never.build(); never._planner._call = 50
    np.testing.assert_array_equal(never.generate_action(st), plain.got)
    assert never.last_recovered is False and never._cost_planner is None


def test_generate_actions_recovers_exactly_the_rows_below_the_threshold():
    _torch()
    states = _states(3)
    _, _, plain = _policy()
    pl = plain.build_batch(3)
    pl._call = 50
    want = plain.generate_actions(states)
    scores = plain.last_scores.copy()
    assert np.unique(scores).size == 3
    thr = float(np.sort(scores)[2])                                            # strictly above two of the three scores
    _, _, rec = _policy(recover_below=thr)
    rec.build_batch(3)._call = 50
    got = rec.generate_actions(states)
    low = scores < thr
    assert low.sum() == 2 and (rec.last_recovered == low).all()
    np.testing.assert_array_equal(got[~low], want[~low])
    np.testing.assert_array_equal(rec.last_calls, np.arange(50, 53, dtype=np.uint64))
    for b in np.nonzero(low)[0]:                                               # each replaced row: the single cost plan with the replaced plan's call number
        np.testing.assert_array_equal(got[b], rec.optimize_for_safety(states[b], call=50 + int(b)))
        assert not np.array_equal(got[b], want[b])
    _, _, off = _policy(recover_below=None)
    off.build_batch(3)._call = 50
    np.testing.assert_array_equal(off.generate_actions(states), want)
    assert not off._cost_batch_planners and off.last_recovered is None
