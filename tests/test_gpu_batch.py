"""Batched planning on the MI355X (cem_planner_plan_batch, BatchCemPlanner, CemMpc.generate_actions).

Every problem of a batched plan must return, bit for bit, what a single-state plan of that problem returns on a handle of the same
configuration (action, best score, iteration count) — at the reference's shipped shapes and BASELINE B2, for both objectives, on the
captured-graph and the eager path, with the sampler in the rollout tiles and as a launch of its own.  Beyond that: the oracle on
explicit and on dumped Philox noise, per-problem early stop, one captured graph for every n_states, the launch count of a batched
iteration, the error paths and the simba-level plugin."""
import ctypes as C

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import helpers as hp

pytestmark = pytest.mark.gpu

# (E = P = ... of the shipped policies: config.py cem_mpc / safe_cem_mpc, ensemble of 15; B2: BASELINE config 2)
SHAPES = {
    'cem_mpc': dict(E=15, P=5, N=150, H=8, k=15, I=10, thr=0.25),
    'safe_cem_mpc': dict(E=15, P=45, N=500, H=8, k=20, I=9, thr=0.25),
    'B2': dict(E=5, P=5, N=2000, H=30, k=200, I=5, thr=-1.0),
}


def _problem(E):
    return hp.make_problem(60, 2, E, 4, seed=1234)


def _cfgs(pb, shape, variant, use_graph, **kw):
    s = dict(SHAPES[shape])
    s.update(kw)
    return hp.configs(pb, N=s['N'], H=s['H'], P=s['P'], E=s['E'], k=s['k'], I=s['I'], variant=variant, thr=s['thr'], noise=1e-3,
                      post=0.2, use_graph=use_graph)


def _batch(pb, pcfg, max_batch):
    from ethz_safe_learning_amd import BatchCemPlanner
    pl = BatchCemPlanner(pcfg, max_batch)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


def _states(pb, n, seed):
    rng = np.random.default_rng(seed)
    st = np.repeat(pb['state'][None], n, 0).astype(np.float32)
    st[1:] += rng.normal(0.0, 0.05, st[1:].shape).astype(np.float32)      # problem 0: the problem's own state
    return st


def _singles(single, states, seed, calls):
    out = [single.plan(states[b], seed=seed, call=int(calls[b])) for b in range(len(states))]
    return (np.stack([a for a, _, _ in out]), np.array([s for _, s, _ in out], np.float32), np.array([i for _, _, i in out], np.int32))


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg='%s: actions' % what)
    np.testing.assert_array_equal(got[1], want[1], err_msg='%s: scores' % what)
    np.testing.assert_array_equal(got[2], want[2], err_msg='%s: iterations' % what)


@pytest.mark.parametrize('sampler', ['tile', 'kernel'])
@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('shape', sorted(SHAPES))
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_every_problem_is_bit_identical_to_its_single_plan(monkeypatch, variant, shape, use_graph, sampler):
    monkeypatch.setenv('CEM_FORCE_SAMPLER', sampler)          # read at handle creation: both handles below
    pb = _problem(SHAPES[shape]['E'])
    _, pcfg = _cfgs(pb, shape, variant, use_graph)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, 8)
    assert pl.batch_capacity() == 8
    for B, seed in ((1, 3), (3, 5), (8, 7)):
        states = _states(pb, B, seed=B)
        calls = np.arange(B, dtype=np.uint64) * 7 + 11
        got = pl.plan_batch(states, seed=seed, calls=calls)
        _assert_same(got, _singles(single, states, seed, calls), '%s %s B=%d graph=%s sampler=%s' % (variant, shape, B, use_graph, sampler))
        assert np.all(np.isfinite(got[0])) and np.all(got[2] >= 1)
    if use_graph:
        assert pl.graph_status() == 'graph' and single.graph_status() == 'graph'
    pl.close()
    single.close()


def test_sixty_four_problems_at_the_shipped_cem_shape():
    pb = _problem(15)
    _, pcfg = _cfgs(pb, 'cem_mpc', 'cem', True)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, 64)
    states = _states(pb, 64, seed=64)
    calls = np.arange(64, dtype=np.uint64) + 1000
    _assert_same(pl.plan_batch(states, seed=9, calls=calls), _singles(single, states, 9, calls), 'cem_mpc B=64')
    assert pl.graph_status() == 'graph'


def test_explicit_noise_problems_match_the_oracle():
    """B = 4 different states, each with its own slice of explicit noise tensors: each problem against oracle.do_generate_action on its
    slice, to smoke()'s tolerances — and bit for bit against single plans on the same slices."""
    pb = hp.make_problem(seed=7)
    N, H, P, E, k, I = 128, 8, 5, 5, 12, 3
    for variant in ('cem', 'safe'):
        ocfg, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=k, I=I, variant=variant, noise=0.01, post=0.3)
        single = hp.make_planner(pb, pcfg)
        pl = _batch(pb, pcfg, 4)
        states = _states(pb, 4, seed=21)
        ns = [hp.noise(I, N, H, 2, P, 60, seed=30 + b) for b in range(4)]
        ea, em, eo = (np.stack([n[i] for n in ns]) for i in range(3))
        acts, scores, iters = pl.plan_batch(states, eps_act=ea, eps_model=em, eps_out=eo, calls=np.zeros(4, np.uint64))
        for b in range(4):
            ra, rs, rit = o.do_generate_action(states[b], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'],
                                               ea[b], em[b], eo[b], ocfg, pb['scorer'])
            assert iters[b] == rit and abs(scores[b] - rs) <= 2e-5, (variant, b, scores[b], rs)
            assert np.allclose(acts[b], ra, rtol=1e-5, atol=1e-6), (variant, b, acts[b], ra)
            a1, s1, i1 = single.plan(states[b], eps_act=ea[b], eps_model=em[b], eps_out=eo[b])
            np.testing.assert_array_equal(acts[b], a1)
            assert scores[b] == np.float32(s1) and iters[b] == i1
        assert len({tuple(a) for a in acts}) == 4              # four different problems


def test_b2_philox_problems_match_the_oracle_in_the_first_iteration():
    """BASELINE B2 on the Philox path, 2 problems (seed 1, calls 3 and 4): the streams each consumed, dumped with cem_fill_noise per
    call, replayed by the oracle.  Iteration 0 (I = 1): every candidate's score, the elite set and mu / sigma of each problem's slice,
    and the returned action, with test_gpu_whole_plan.py's tolerances."""
    import torch
    pb = hp.make_problem(60, 2, 5, 4, seed=1234, bias_noise=0.0)
    N, k = 2000, 200
    ocfg, pcfg = hp.configs(pb, N=N, H=30, P=5, E=5, k=k, I=1, variant='cem', noise=1e-3, post=0.3, use_graph=True)
    pl = _batch(pb, pcfg, 2)
    single = hp.make_planner(pb, pcfg)
    states = np.repeat(pb['state'][None], 2, 0)
    calls = np.array([3, 4], np.uint64)
    acts, scores, iters = pl.plan_batch(states, seed=1, calls=calls)
    pl.synchronize()
    sc = pl._view(pl.layout.scores_local, 2 * N, torch.float32).view(2, N).cpu().numpy()
    el = pl._view(pl.layout.elite_idx, 2 * k, torch.int32).view(2, k).cpu().numpy()
    ms = pl._view(pl.layout.mu_sigma, 2 * 2 * 30 * 2, torch.float32).view(2, 2, 30, 2).cpu().numpy()
    for b in range(2):
        ea, em, eo = single.fill_noise(seed=1, call=int(calls[b]))
        trace = []
        ra, rs, rit = o.do_generate_action(states[b], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'],
                                           ea.cpu().numpy(), em.cpu().numpy(), eo.cpu().numpy(), ocfg, pb['scorer'], trace=trace)
        del ea, em, eo
        diff = np.abs(sc[b] - trace[0]['scores'])
        flipped = diff > 2e-5 + 6e-8 * np.abs(trace[0]['scores'])
        assert flipped.mean() <= 0.03, (b, int(flipped.sum()))
        assert hp.elite_sets_equal_modulo_ties(trace[0]['scores'], np.sort(el[b]), trace[0]['elite'], 2e-5), b
        if np.array_equal(np.sort(el[b]), np.sort(trace[0]['elite'])):
            np.testing.assert_allclose(ms[b, 0], trace[0]['mu'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(ms[b, 1], trace[0]['sigma'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(acts[b], ra, rtol=1e-5, atol=1e-7)
            assert abs(scores[b] - rs) <= 2e-5 + 6e-8 * abs(rs)
        assert iters[b] == rit == 1
        torch.cuda.empty_cache()


def test_problems_stop_early_each_on_their_own():
    """stddev_threshold and states such that the problems of one batch stop at different iterations (>= 3 distinct counts), each
    equal to its single plan's; a problem that has stopped is not touched by the iterations the others still run (its mu / sigma
    slice equals the single plan's final one)."""
    import torch
    pb = _problem(15)
    found = None
    for thr in (0.25, 0.3, 0.2, 0.35, 0.15, 0.4):
        _, pcfg = _cfgs(pb, 'cem_mpc', 'cem', True, thr=thr)
        pl = _batch(pb, pcfg, 16)
        states = _states(pb, 16, seed=99)
        states[8:] = np.random.default_rng(5).uniform(0.0, 1.0, states[8:].shape).astype(np.float32)
        calls = np.arange(16, dtype=np.uint64) * 3 + 1
        got = pl.plan_batch(states, seed=2, calls=calls)
        if len(set(got[2].tolist())) >= 3:
            found = (thr, pcfg, pl, states, calls, got)
            break
        pl.close()
    assert found is not None, 'no threshold gave three distinct iteration counts'
    thr, pcfg, pl, states, calls, got = found
    assert got[2].min() < SHAPES['cem_mpc']['I']
    single = hp.make_planner(pb, pcfg)
    _assert_same(got, _singles(single, states, 2, calls), 'early stop thr=%g' % thr)
    pl.synchronize()
    HA = 8 * 2
    ms = pl._view(pl.layout.mu_sigma, 16 * 2 * HA, torch.float32).view(16, 2 * HA).cpu().numpy()
    for b in np.argsort(got[2])[:4]:                          # the earliest stoppers
        single.plan(states[b], seed=2, call=int(calls[b]))
        np.testing.assert_array_equal(ms[b], single.mu_sigma().cpu().numpy().reshape(-1), err_msg='problem %d' % b)


def test_one_graph_serves_every_batch_size():
    pb = _problem(15)
    _, pcfg = _cfgs(pb, 'cem_mpc', 'safe', True)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, 8)
    for i, n in enumerate((8, 3, 8, 1)):
        states = _states(pb, n, seed=40 + i)
        calls = np.arange(n, dtype=np.uint64) + 100 * i
        _assert_same(pl.plan_batch(states, seed=4, calls=calls), _singles(single, states, 4, calls), 'n_states %d' % n)
        assert pl.graph_status() == 'graph'


def test_a_batched_iteration_is_one_launch_per_stage():
    pb = _problem(15)
    for variant in ('cem', 'safe'):
        _, pcfg = _cfgs(pb, 'cem_mpc', variant, True)
        pl = _batch(pb, pcfg, 8)
        n0 = pl.launches_per_iteration()
        assert 2 <= n0 <= 4
        pl.set_timing(True)
        for n in (1, 8):
            pl.plan_batch(_states(pb, n, seed=n), seed=1)
            t = pl.last_timing()
            assert t['rollout_launches'] == SHAPES['cem_mpc']['I'], (variant, n, t)
            assert pl.launches_per_iteration() == n0
        pl.set_timing(False)


def test_error_paths_leave_the_handle_usable():
    from ethz_safe_learning_amd._capi import CemError
    pb = _problem(15)
    _, pcfg = _cfgs(pb, 'cem_mpc', 'cem', True)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, 4)
    states = _states(pb, 4, seed=1)
    calls = np.arange(4, dtype=np.uint64)
    want = _singles(single, states, 0, calls)
    _assert_same(pl.plan_batch(states, calls=calls), want, 'before')
    for bad in (np.zeros((0, 60), np.float32), _states(pb, 5, seed=2)):
        with pytest.raises(CemError) as e:
            pl.plan_batch(bad)
        assert e.value.status == 1
        _assert_same(pl.plan_batch(states, calls=calls), want, 'after n_states %d' % len(bad))
    with pytest.raises(CemError) as e:                         # single-state calls on a batch handle
        pl.plan(pb['state'])
    assert e.value.status == 7
    with pytest.raises(CemError) as e:
        pl.plan_begin(pb['state'])
    assert e.value.status == 7
    with pytest.raises(CemError) as e:
        pl.compute_objective(np.zeros((5, 9, 60), np.float32))
    assert e.value.status == 7
    _assert_same(pl.plan_batch(states, calls=calls), want, 'after single-state calls')
    # the batched call on a single-state handle
    cl = (C.c_uint64 * 1)()
    st = np.ascontiguousarray(states[:1])
    out_a, out_s, out_i = np.zeros(2, np.float32), np.zeros(1, np.float32), np.zeros(1, np.int32)
    assert single.lib.cem_planner_plan_batch(single.h, 1, st.ctypes.data_as(C.c_void_p), 0, cl, None, None, None,
                                             out_a.ctypes.data_as(C.c_void_p), out_s.ctypes.data_as(C.c_void_p),
                                             out_i.ctypes.data_as(C.c_void_p)) == 7
    n = C.c_int32(-1)
    assert single.lib.cem_planner_batch_capacity(single.h, C.byref(n)) == 0 and n.value == 0
    a, s, i = single.plan(states[0], seed=0, call=0)
    np.testing.assert_array_equal(a, want[0][0])


@pytest.mark.parametrize('policy_name', ['cem_mpc', 'safe_cem_mpc'])
def test_policy_generate_actions_equals_generate_action(policy_name):
    from tests.test_simba_api import make_agent_parts, trained_like
    env, model, pol = make_agent_parts(policy_name, seed=3)
    rng = np.random.default_rng(0)
    trained_like(model, rng)
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    states = np.stack([PointGoalEnv(seed=s).reset() for s in range(3)]).astype(np.float32)      # (the same observation layout)

    def per_state():
        pol.build()
        pol._planner._call = 50
        return np.stack([pol.generate_action(s) for s in states])

    want = per_state()
    pl = pol.build_batch(3)
    assert pl.max_batch == 4
    pl._call = 50
    got = pol.generate_actions(states)
    np.testing.assert_array_equal(got, want)
    assert pol.last_scores.shape == (3,) and pol.last_iterations.shape == (3,)
    # a model update (version bump) re-stages the batch handle's weights / normaliser
    trained_like(model, np.random.default_rng(1))
    want2 = per_state()
    pl._call = 50
    got2 = pol.generate_actions(states)
    assert pl.staged == (model.uid, model.version)
    np.testing.assert_array_equal(got2, want2)
    assert not np.array_equal(got2, got)


def test_lockstep_evaluation_on_four_environments():
    from tests.test_simba_api import make_agent_parts, trained_like
    from ethz_safe_learning_amd.simba.agents.agent import BaseAgent
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    env, model, pol = make_agent_parts('cem_mpc', seed=4)
    trained_like(model, np.random.default_rng(2))
    envs = [PointGoalEnv(n_hazards=8, n_vases=1, num_steps=12, seed=s, config=dict(constrain_hazards=True)) for s in range(4)]
    agent = BaseAgent(replay_buffer_size=100, add_observation_noise=False, action_repeat=2)
    paths, steps = agent.sample_trajectories_lockstep(envs, pol, batch_size=1, max_trajectory_length=12)
    assert len(paths) == 4 and steps == 4 * 12
    for p in paths:
        n = len(p['action'])                                  # 6 decisions of 2 steps (more if a goal cut a hold short)
        assert 6 <= n <= 12 and p['action'].shape == (n, 2) and p['observation'].shape == (n, env.observation_space.shape[0])
        assert np.all(np.isfinite(p['action'])) and np.all(np.abs(p['action']) <= 1.01)      # (the output noise is added after the clip, cem_mpc.py:68)
        assert p['terminal'][-1] == 1.0 and len(p['info']) == n
