"""Time-correlated action noise (cem_planner_set_action_noise, CEM_NOISE_MIXED) on the device.

The feature has a bit-exact reference that costs nothing: the white streams the mix kernel draws are the ones fill_noise dumps, the
contract's sum is planner.mix_noise, and a plan fed an eps_act tensor is an existing, separately tested path.  So
  the kernel alone     action_noise_tensor() == mix_noise(M, fill_noise(seed, call).eps_act), every matrix of tests/colored_cases.py
  whole plans          a MIXED plan on Philox noise == a WHITE handle fed eps_act = mix_noise(M, white) and the dumped model / output noise
and everything else (the oracle, M = I, routing, batch, warm start, refusals, the policies) hangs off those two."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd.planner import ar1_mixing, mix_noise, powerlaw_mixing
from tests import colored_cases as cc
from tests import helpers as hp

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
FULL_SIZE_ATOL = 2e-5                    # tests/test_gpu_parity.py: the score bar of its tensor-fed whole plans against the oracle
N, H, P, E, K, I = 64, 8, 5, 5, 8, 3     # the whole-plan shape
SEED, CALL = 5, 9
_PB = {}


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _pb(units=128, A=2):
    if (units, A) not in _PB:
        _PB[(units, A)] = hp.make_problem(seed=42, units=units, act_dim=A)
    return _PB[(units, A)]


def _cfg(pb, variant='cem', n=N, h=H, k=K, i=I, **kw):
    return hp.configs(pb, N=n, H=h, P=P, E=E, k=k, I=i, variant=variant, noise=0.01, post=0.3, **kw)


def _left(pl):
    """What a plan leaves on the device."""
    return dict(mu_sigma=_np(pl.mu_sigma()), elite_idx=_np(pl.elite_idx()), actions=_np(pl.actions()))


def _same_plan(got, want, left_got, left_want, what):
    np.testing.assert_array_equal(got[0].view(U), want[0].view(U), err_msg='%s: action' % what)
    assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2], (what, got, want)
    for key in ('mu_sigma', 'elite_idx', 'actions'):
        a, b = left_got[key], left_want[key]
        np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg='%s: %s' % (what, key))


def _fed(white, M, state, seed, call):
    """The reference: the WHITE handle fed eps_act = mix_noise(M, its own dumped white stream) and the dumped model / output noise."""
    ea, em, eo = white.fill_noise(seed=seed, call=call)
    eps = mix_noise(M, _np(ea))
    r = white.plan(state, seed=seed, call=call, eps_act=eps, eps_model=em, eps_out=_np(eo))
    return r, _left(white), eps


# ------------------------------------------------------------------------------------------------- 1: the kernel alone
def _kernel_alone(M, n, h, a, i):
    _torch()
    pb = _pb(A=a)
    _, pcfg = _cfg(pb, n=n, h=h, k=max(2, n // 8), i=i)
    pl = hp.make_planner(pb, pcfg)
    try:
        assert pl.action_noise() == ('white', None) and pl.action_noise_floats() == 0
        pl.set_action_noise(M)
        kind, back = pl.action_noise()
        assert kind == 'mixed' and np.array_equal(back.view(U), M.view(U))
        assert pl.action_noise_floats() == i * n * h * a
        assert not pl.action_noise_tensor().any()                                # zeros until a MIXED plan has run
        for seed, call in ((SEED, CALL), (SEED + 1, (3 << 32) + 1)):             # (a call number with high bits: the key's second word)
            pl.plan(pb['state'], seed=seed, call=call)
            got = pl.action_noise_tensor()
            white = _np(pl.fill_noise(seed=seed, call=call)[0])
            assert got.shape == white.shape == (i, n, h, a)
            np.testing.assert_array_equal(got.view(U), mix_noise(M, white).view(U))
    finally:
        pl.close()


@pytest.mark.parametrize('name', cc.MATRIX_NAMES)
def test_kernel_alone_every_matrix(name):
    n, h, a, i = cc.BASE_SHAPE
    _kernel_alone(cc.matrix(name, h), n, h, a, i)


@pytest.mark.parametrize('shape', cc.EXTRA_SHAPES, ids=lambda s: 'N%d_H%d_A%d_I%d' % s)
def test_kernel_alone_shapes(shape):
    n, h, a, i = shape
    _kernel_alone(cc.matrix('dense', h), n, h, a, i)


# ------------------------------------------------------------------------------------------------- 2: whole plans against the tensor path
@pytest.mark.parametrize('variant,precision,units,matrix', [('cem', 'fp32', 128, 'ar1_0.9'), ('safe', 'fp32', 128, 'dense'),
                                                            ('cem', 'bf16x3', 128, 'powerlaw_2'), ('safe', 'fp32', 256, 'ar1_0.5')],
                         ids=['cem', 'safe', 'bf16x3', 'wide256'])
def test_mixed_plans_equal_the_tensor_fed_white_plan(variant, precision, units, matrix):
    torch = _torch()
    pb = _pb(units)
    M = cc.matrix(matrix, H)
    _, pcfg = _cfg(pb, variant, precision=precision)
    white = hp.make_planner(pb, pcfg)
    want = {c: _fed(white, M, pb['state'], SEED, c) for c in (CALL, CALL + 1)}
    # eager
    pl = hp.make_planner(pb, pcfg)
    pl.set_action_noise(M)
    got = pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == 'eager'
    _same_plan(got, want[CALL][0], _left(pl), want[CALL][1], 'eager')
    np.testing.assert_array_equal(pl.action_noise_tensor().view(U), want[CALL][2].view(U))
    # stepwise: cem_plan_begin runs the mix
    pl.plan_begin(pb['state'], seed=SEED, call=CALL + 1)
    for it in range(I):
        pl.plan_rollout(it)
        pl.plan_select(it)
    got = pl.plan_end()
    _same_plan(got, want[CALL + 1][0], _left(pl), want[CALL + 1][1], 'stepwise')
    pl.close()
    # a captured graph, two consecutive plans through it
    pg = hp.make_planner(pb, dataclasses.replace(pcfg, use_graph=True))
    pg.set_action_noise(M)
    for c in (CALL, CALL + 1):
        got = pg.plan(pb['state'], seed=SEED, call=c)
        assert pg.graph_status() == 'graph'
        _same_plan(got, want[c][0], _left(pg), want[c][1], 'graph call %d' % c)
    np.testing.assert_array_equal(pg.action_noise_tensor().view(U), want[CALL + 1][2].view(U))
    # and a caller's own eps_act is taken as given, not mixed, on a MIXED handle too
    ea, em, eo = white.fill_noise(seed=SEED, call=CALL)
    fed_white = white.plan(pb['state'], seed=SEED, call=CALL, eps_act=ea, eps_model=em, eps_out=_np(eo))
    fed_mixed = pg.plan(pb['state'], seed=SEED, call=CALL, eps_act=ea, eps_model=em, eps_out=_np(eo))
    left_white = _left(white)
    _same_plan(fed_mixed, fed_white, _left(pg), left_white, 'caller tensors on a MIXED handle')
    # (the mix is live: the white plan refits another distribution.  Not held on the returned action: with a triangular M step 0 of every
    # sequence is the white draw, and the best candidate of both plans can be the same one)
    assert not np.array_equal(left_white['mu_sigma'], want[CALL][1]['mu_sigma'])
    torch.cuda.synchronize()
    pg.close(); white.close()


# ------------------------------------------------------------------------------------------------- 3: the oracle
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_mixed_plan_agrees_with_the_oracle_fed_the_mixed_tensor(variant):
    """tests/test_gpu_parity.py::test_full_plan_matches_oracle with the MIXED plan in the device's place: per iteration the clipped actions,
    the scores (a row that crosses a `<=` threshold on one side only must be rare), the elite set (modulo near ties), mu / sigma; then the
    action to 1e-5 relative and the score to FULL_SIZE_ATOL — that test's shape and bars."""
    torch = _torch()
    pb = hp.make_problem(seed=51)
    n, h, k, i = 160, 10, 16, 4
    ocfg, pcfg = hp.configs(pb, N=n, H=h, P=P, E=E, k=k, I=i, variant=variant, noise=0.01, post=0.3)
    M = ar1_mixing(h, 0.9)
    pl = hp.make_planner(pb, pcfg)
    pl.set_action_noise(M)
    ea, em, eo = (_np(t) for t in pl.fill_noise(seed=SEED, call=CALL))
    trace = []
    ra, rs, rit = o.do_generate_action(pb['state'], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'],
                                       mix_noise(M, ea), em, eo, ocfg, pb['scorer'], trace=trace)
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    elites_match = True
    for it in range(i):
        pl.plan_rollout(it)
        torch.cuda.synchronize()
        scores = _np(pl.scores_local())
        if elites_match:
            np.testing.assert_allclose(_np(pl.actions()), trace[it]['actions'], rtol=1e-5, atol=1e-6)
            bad = np.abs(scores - trace[it]['scores']) > FULL_SIZE_ATOL
            assert bad.mean() < 0.05, 'iteration %d: %d/%d scores differ' % (it, bad.sum(), n)
        pl.plan_select(it)
        torch.cuda.synchronize()
        elite = _np(pl.elite_idx())
        if elites_match and set(elite.tolist()) != set(trace[it]['elite'].tolist()):
            assert hp.elite_sets_equal_modulo_ties(trace[it]['scores'], elite, trace[it]['elite'], FULL_SIZE_ATOL)
            elites_match = False          # a near-tie flipped: later iterations legitimately diverge
        if elites_match:
            ms = _np(pl.mu_sigma())
            np.testing.assert_allclose(ms[0], trace[it]['mu'], rtol=1e-5, atol=1e-6)
            np.testing.assert_allclose(ms[1], trace[it]['sigma'], rtol=1e-5, atol=1e-6)
    a, s, it = pl.plan_end()
    pl.close()
    assert it == rit == i
    assert elites_match, 'an elite set differed from the oracle (a near-tie on the k-th score?)'
    np.testing.assert_allclose(a, ra, rtol=1e-5, atol=1e-7)
    assert abs(s - rs) <= FULL_SIZE_ATOL


# ------------------------------------------------------------------------------------------------- 4: identity
LEAN = dict(N=40, H=3, P=2, E=2, k=4, I=2, post=0.3, chunks_per_tile=1)            # tests/test_gpu_lean_rollout.py's lean-eligible shape


@pytest.mark.parametrize('sampler,segments,variant', [('tile', 1, 'cem'), ('tile', 3, 'cem'), ('kernel', 1, 'safe')],
                         ids=['tile_prologue', 'floating_segment_prologue', 'sampler_launch'])
def test_identity_matrix_is_the_generic_white_plan(monkeypatch, sampler, segments, variant):
    """M = I through the generic sampler in its three places.  The only divergence the contract allows is a white draw of exactly -0.0,
    which mixes to +0.0; in the clipped actions (-0 sigma + mu == +0 sigma + mu) it vanishes, and those are what is compared."""
    _torch()
    pb = hp.make_problem(60, 2, 2, 4, seed=77)
    monkeypatch.setenv('CEM_FORCE_SAMPLER', sampler)
    _, pcfg = hp.configs(pb, use_graph=True, variant=variant, rollout_segments=segments, **LEAN)
    monkeypatch.setenv('CEM_FORCE_ROLLOUT', 'generic')
    white = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT')
    mixed = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_SAMPLER')
    assert white.rollout_path() == 'generic' and (white.segments()[0] > 1) == (segments > 1)
    mixed.set_action_noise(np.eye(LEAN['H'], dtype=F))
    assert mixed.rollout_path() == 'generic' and mixed.launches_per_iteration() == white.launches_per_iteration()
    for c in (CALL, CALL + 1):
        got, want = mixed.plan(pb['state'], seed=SEED, call=c), white.plan(pb['state'], seed=SEED, call=c)
        assert mixed.graph_status() == white.graph_status() == 'graph'
        _same_plan(got, want, _left(mixed), _left(white), 'identity call %d' % c)
    mixed.close(); white.close()


# ------------------------------------------------------------------------------------------------- 5: routing
def test_routing_lean_generic_and_back():
    torch = _torch()
    pb = hp.make_problem(60, 2, 2, 4, seed=77)
    _, pcfg = hp.configs(pb, use_graph=True, **LEAN)
    pl, fresh = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    base = fresh.launches_per_iteration()
    assert pl.rollout_path() == fresh.rollout_path() == 'lean' and pl.launches_per_iteration() == base
    pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == 'graph'
    M = ar1_mixing(LEAN['H'], 0.9)
    pl.set_action_noise(M)
    assert pl.rollout_path() == 'generic' and pl.launches_per_iteration() == base and pl.graph_status() == 'eager'
    pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == 'graph'
    mixed_ms = _np(pl.mu_sigma())
    pl.set_action_noise('white')
    assert pl.action_noise() == ('white', None) and pl.rollout_path() == 'lean' and pl.launches_per_iteration() == base
    assert pl.graph_status() == 'eager'
    got, want = pl.plan(pb['state'], seed=SEED, call=CALL), fresh.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == fresh.graph_status() == 'graph'
    _same_plan(got, want, _left(pl), _left(fresh), 'back on white')
    for view in ('scores_local', 'returns'):
        assert torch.equal(getattr(pl, view)(), getattr(fresh, view)()), view
    assert not np.array_equal(mixed_ms, _np(fresh.mu_sigma()))                    # (the mixed plan was another plan)
    pl.set_action_noise('powerlaw', 2.0)                                          # the named kinds go through the helpers
    assert np.array_equal(pl.action_noise()[1], powerlaw_mixing(LEAN['H'], 2.0))
    pl.set_action_noise('ar1', 0.5)
    assert np.array_equal(pl.action_noise()[1], ar1_mixing(LEAN['H'], 0.5))
    pl.close(); fresh.close()


# ------------------------------------------------------------------------------------------------- 6: batch
def test_batch_rows_are_their_single_mixed_plans():
    _torch()
    from ethz_safe_learning_amd import BatchCemPlanner
    pb = _pb()
    M = cc.matrix('dense', H)
    _, pcfg = _cfg(pb, 'safe', use_graph=True)
    rng = np.random.default_rng(3)
    states = (pb['state'][None] + rng.normal(0, 0.05, (4, pb['state'].shape[0]))).astype(F)
    bp = BatchCemPlanner(pcfg, 4)
    bp.set_weights(pb['weights']); bp.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    bp.set_action_noise(M)
    assert bp.action_noise_floats() == 4 * I * N * H * 2
    bp.plan_batch(states, seed=SEED, calls=np.array([20, 21, 22, 23], np.uint64))      # all four: every slice of the buffer is written
    before = [bp.action_noise_tensor(b) for b in range(4)]
    assert all(t.any() for t in before)
    calls = np.array([4, 5, 6], np.uint64)
    acts, scores, iters = bp.plan_batch(states[:3], seed=SEED, calls=calls)             # three problems, the fourth staged as stopped
    assert bp.graph_status() == 'graph'
    one = hp.make_planner(pb, pcfg)
    one.set_action_noise(M)
    for b in range(3):
        a, s, i = one.plan(states[b], seed=SEED, call=int(calls[b]))
        np.testing.assert_array_equal(acts[b].view(U), a.view(U))
        assert F(scores[b]).view(U) == F(s).view(U) and iters[b] == i
        np.testing.assert_array_equal(bp.action_noise_tensor(b).view(U), one.action_noise_tensor().view(U))
        assert not np.array_equal(bp.action_noise_tensor(b), before[b])
    np.testing.assert_array_equal(bp.action_noise_tensor(3).view(U), before[3].view(U))      # the stopped problem's slice keeps its bytes
    with pytest.raises(ValueError):
        bp.action_noise_tensor(4)
    bp.close(); one.close()


# ------------------------------------------------------------------------------------------------- 7: warm start
def test_shift_started_mixed_plan_equals_the_tensor_fed_one():
    _torch()
    pb = _pb()
    M = cc.matrix('ar1_0.9', H)
    _, pcfg = _cfg(pb, 'cem', use_graph=True)
    pl, white = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    pl.set_action_noise(M)
    for p in (pl, white):
        p.set_warm_start(shift=1, sigma='keep', floor_frac=0.1)
        p.set_init_mode('shift')
    for c in (CALL, CALL + 1):                                                    # a cold plan, then one from its shifted carry
        got = pl.plan(pb['state'], seed=SEED, call=c)
        want, left, _ = _fed(white, M, pb['state'], SEED, c)
        _same_plan(got, want, _left(pl), left, 'warm call %d' % c)
        for x, y in zip(pl.carry(0), white.carry(0)):
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y))
    cold = hp.make_planner(pb, pcfg)
    cold.set_action_noise(M)
    cold.plan(pb['state'], seed=SEED, call=CALL + 1)
    assert not np.array_equal(_np(cold.mu_sigma()), _np(pl.mu_sigma()))          # (the second plan did start warm)
    pl.close(); white.close(); cold.close()


# ------------------------------------------------------------------------------------------------- 8: refusals
def _status(fn, *a, **kw):
    from ethz_safe_learning_amd._capi import CemError
    with pytest.raises(CemError) as e:
        fn(*a, **kw)
    return e.value.status


def test_refusals():
    _torch()
    pb = _pb()
    M = ar1_mixing(H, 0.5)
    # a sharded configuration
    pl = hp.make_planner(pb, _cfg(pb, world_size=2, rank=0)[1])
    assert _status(pl.set_action_noise, M) == UNSUPPORTED and pl.action_noise() == ('white', None) and pl.action_noise_floats() == 0
    pl.set_action_noise('white')                                                 # the default is always accepted
    pl.close()
    with pytest.raises(Exception):
        hp.make_planner(pb, dataclasses.replace(_cfg(pb, world_size=2, rank=0)[1], action_noise='ar1', action_noise_param=0.5))
    # a horizon beyond the kernel's LDS
    pl = hp.make_planner(pb, _cfg(pb, n=16, h=129, k=2, i=1)[1])
    assert _status(pl.set_action_noise, np.eye(129, dtype=F)) == UNSUPPORTED and pl.action_noise_floats() == 0
    a, s, i = pl.plan(pb['state'], seed=1, call=0)                               # ... and the handle still plans
    assert np.isfinite(a).all() and i == 1
    pl.close()
    pl = hp.make_planner(pb, _cfg(pb)[1])
    for bad in (np.nan, np.inf, -np.inf):
        Mb = M.copy(); Mb[H - 1, 2] = bad
        assert _status(pl.set_action_noise, Mb) == INVALID_ARG
    lib, ptr = pl.lib, M.ctypes.data_as(C.c_void_p)
    assert lib.cem_planner_set_action_noise(pl.h, 1, None) == INVALID_ARG         # MIXED with NULL
    assert lib.cem_planner_set_action_noise(pl.h, 0, ptr) == INVALID_ARG          # WHITE with a matrix
    assert lib.cem_planner_set_action_noise(pl.h, 2, ptr) == INVALID_ARG
    assert pl.action_noise() == ('white', None) and pl.action_noise_floats() == 0
    with pytest.raises(RuntimeError):
        pl.action_noise_tensor()
    # inside a stepwise plan
    pl.set_action_noise(M)
    pl.plan_begin(pb['state'], seed=1, call=0)
    assert _status(pl.set_action_noise, 'white') == STATE
    assert _status(pl.set_action_noise, cc.matrix('dense', H)) == STATE
    for it in range(I):
        pl.plan_rollout(it); pl.plan_select(it)
    a, s, i = pl.plan_end()
    assert pl.action_noise()[0] == 'mixed' and np.array_equal(pl.action_noise()[1], M) and i == I and np.isfinite(a).all()
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


@pytest.mark.parametrize('name,extra,matrix', [('cem_mpc', dict(noise_beta=2.0), powerlaw_mixing), ('safe_cem_mpc', dict(noise_rho=0.9), ar1_mixing)],
                         ids=['cem_beta', 'safe_rho'])
def test_policies_plan_with_correlated_noise(name, extra, matrix):
    _torch()
    states = _states(3)
    env, pol = _policy(name, **extra)
    cfg = pol.planner_config()
    want = matrix(cfg.horizon, list(extra.values())[0])
    assert (cfg.action_noise, cfg.action_noise_param) == (('powerlaw', 2.0) if 'noise_beta' in extra else ('ar1', 0.9))
    pol.build_batch(3)._call = 50
    acts = pol.generate_actions(states)
    assert acts.shape == (3, 2) and (acts >= env.action_space.low - 0.1).all() and (acts <= env.action_space.high + 0.1).all()
    bp = pol.build_batch(3)
    assert bp.action_noise()[0] == 'mixed' and np.array_equal(bp.action_noise()[1].view(U), want.view(U))
    for b in range(3):
        pol.build(); pol._planner._call = 50 + b
        a = pol.generate_action(states[b])
        kind, M = pol._planner.action_noise()
        assert kind == 'mixed' and np.array_equal(M.view(U), want.view(U)) and pol._planner.graph_status() == 'graph'
        assert pol._planner.rollout_path() == 'generic'
        np.testing.assert_array_equal(a.view(U), acts[b].view(U))                  # a row of the batch is its single plan
    if name == 'safe_cem_mpc':                                                    # the cost plans follow the policy's setting
        assert pol.cost_planner_config().action_noise == 'ar1'
        pol.optimize_for_safety(states[0], call=1)
        assert pol._cost_planner.action_noise()[0] == 'mixed'


def test_policy_without_noise_arguments_is_the_parent_policy():
    _torch()
    from ethz_safe_learning_amd.planner import config_key, planner_cache_info
    st = _states(1)[0]
    _, plain = _policy('cem_mpc')
    plain.build(); plain._planner._call = 50
    a_plain = plain.generate_action(st)
    n_handles = planner_cache_info()['size']
    _, none = _policy('cem_mpc', noise_beta=None, noise_rho=None)
    none.build(); none._planner._call = 50
    assert none._planner is plain._planner and planner_cache_info()['size'] == n_handles
    np.testing.assert_array_equal(none.generate_action(st).view(U), a_plain.view(U))
    assert none.last_score == plain.last_score
    assert none._planner.action_noise() == ('white', None) and none._planner.action_noise_floats() == 0      # no noise buffer
    assert config_key(none.planner_config()) == config_key(plain.planner_config())
    for bad in (dict(noise_beta=1.0, noise_rho=0.5), dict(noise_beta=-1.0), dict(noise_rho=1.0)):
        with pytest.raises(ValueError):
            _policy('cem_mpc', **bad)
