"""Warm start on the MI355X (cem_mpc.h: cem_init_mode).

Cold stays cold (a handle told COLD, or EXPLICIT with the box broadcast, returns an untouched handle's bits); a SHIFT chain equals an
EXPLICIT chain fed with the NumPy shift of the read-back mu / sigma, bit for bit; the chain matches the oracle composed from its own
stages on explicit noise; every problem of a batched chain with a changing slot map equals its slot's single-handle chain; the carry is
dropped where the interface says so; the policy layer."""
import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import helpers as hp
from tests import warm_cases as wc

pytestmark = pytest.mark.gpu

SMALL = dict(E=5, P=5, N=128, H=8, k=12, I=3)
SHAPES = {
    'small': SMALL,
    'cem_mpc': dict(E=15, P=5, N=150, H=8, k=15, I=10),
    'safe_cem_mpc': dict(E=15, P=45, N=500, H=8, k=20, I=9),
    'B2': dict(E=5, P=5, N=2000, H=30, k=200, I=5),
}
TAILS, RULES = ('box', 'repeat'), ('reset', 'keep')


def _setup(shape, variant, thr=-1.0, use_graph=True, units=128, precision='fp32', **kw):
    s = SHAPES[shape]
    pb = hp.make_problem(60, 2, s['E'], 4, seed=7 if shape == 'small' else 1234, units=units)
    ocfg, pcfg = hp.configs(pb, N=s['N'], H=s['H'], P=s['P'], E=s['E'], k=s['k'], I=s['I'], variant=variant, thr=thr, noise=0.01, post=0.3,
                            use_graph=use_graph, precision=precision, **kw)
    return pb, ocfg, pcfg


def _states(pb, n, seed=5, drift=0.02):
    """A drifting observation sequence: the problem's state plus a random walk."""
    rng = np.random.default_rng(seed)
    out, st = [], pb['state'].astype(np.float32).copy()
    for _ in range(n):
        out.append(st.copy())
        st = st + rng.normal(0, drift, st.shape).astype(np.float32)
    return out


def _snapshot(pl, res):
    ms = pl.mu_sigma().cpu().numpy().copy()
    return dict(action=res[0].copy(), score=np.float32(res[1]), iters=int(res[2]), musig=ms, elite=np.sort(pl.elite_idx().cpu().numpy()))


def _same(a, b, what):
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg='%s: %s' % (what, k))


def _floor(pcfg, frac=0.25):
    from ethz_safe_learning_amd.planner import warm_sigma_floor
    return warm_sigma_floor(pcfg, frac)


# ---------------------------------------------------------------------------------------------------------------- 1. cold stays cold
@pytest.mark.parametrize('sampler', ['tile', 'kernel'])
@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('variant,shape', [('cem', 'cem_mpc'), ('safe', 'safe_cem_mpc'), ('cem', 'B2'), ('safe', 'small')])
def test_cold_and_broadcast_explicit_return_an_untouched_handles_bits(monkeypatch, variant, shape, use_graph, sampler):
    monkeypatch.setenv('CEM_FORCE_SAMPLER', sampler)
    pb, _, pcfg = _setup(shape, variant, thr=0.25 if shape != 'B2' else -1.0, use_graph=use_graph)
    plain, cold, expl = (hp.make_planner(pb, pcfg) for _ in range(3))
    cold.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)       # parameters alone change nothing
    cold.set_init_mode('cold')
    mu0, sg0 = wc.box(pb, pcfg.horizon)
    expl.set_initial_distribution(mu0, sg0)
    expl.set_init_mode('explicit')
    for i, st in enumerate(_states(pb, 3)):
        want = _snapshot(plain, plain.plan(st, seed=3, call=i))
        _same(_snapshot(cold, cold.plan(st, seed=3, call=i)), want, 'cold plan %d' % i)
        _same(_snapshot(expl, expl.plan(st, seed=3, call=i)), want, 'explicit box plan %d' % i)
    if use_graph:
        assert cold.graph_status() == 'graph' and expl.graph_status() == 'graph'
    for p in (plain, cold, expl):
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 2. shift equals explicit
def _shift_vs_explicit(pb, pcfg, s, tail, rule, stepwise=False, n_plans=4, seed=11):
    A, B = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    A.set_warm_start(shift=s, tail=tail, sigma=rule, floor_frac=0.25)
    A.set_init_mode('shift')
    B.set_init_mode('explicit')
    mu0, sg0 = wc.box(pb, pcfg.horizon)
    fl = _floor(pcfg)
    prev = None
    iters = []

    def run(pl, st, i):
        if not stepwise:
            return pl.plan(st, seed=seed, call=i)
        pl.plan_begin(st, seed=seed, call=i)
        for it in range(pcfg.iterations):
            pl.plan_rollout(it)
            pl.plan_select(it)
        return pl.plan_end()

    for i, st in enumerate(_states(pb, n_plans)):
        if prev is None:
            B.set_initial_distribution(mu0, sg0)
        else:
            B.set_initial_distribution(*wc.shift(prev[0], prev[1], mu0[0], sg0[0], s, TAILS.index(tail), RULES.index(rule), fl))
        b = _snapshot(B, run(B, st, i))
        a = _snapshot(A, run(A, st, i))
        _same(a, b, 's=%d %s %s plan %d' % (s, tail, rule, i))
        prev = (b['musig'][0], b['musig'][1])
        for pl in (A, B):
            m, g, valid = pl.carry()
            assert valid
            np.testing.assert_array_equal(m, prev[0])
            np.testing.assert_array_equal(g, prev[1])
        iters.append(a['iters'])
    if pcfg.use_graph and not stepwise:
        assert A.graph_status() == 'graph' and B.graph_status() == 'graph'
    A.close()
    B.close()
    return iters


@pytest.mark.parametrize('thr', [-1.0, 0.5])
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('tail', TAILS)
@pytest.mark.parametrize('s', [1, 3])
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_shift_chain_equals_explicit_chain_small(variant, s, tail, rule, thr):
    pb, _, pcfg = _setup('small', variant, thr=thr)
    iters = _shift_vs_explicit(pb, pcfg, s, tail, rule)
    if thr < 0:
        assert iters == [3] * 4


@pytest.mark.parametrize('variant,shape,kw', [
    ('cem', 'cem_mpc', dict(thr=0.25)), ('safe', 'safe_cem_mpc', dict(thr=0.25)), ('cem', 'B2', dict()), ('safe', 'B2', dict()),
    ('cem', 'small', dict(precision='bf16x3')), ('safe', 'small', dict(precision='bf16x3', thr=0.5)),
    ('cem', 'small', dict(units=200)), ('cem', 'small', dict(use_graph=False)), ('safe', 'cem_mpc', dict(use_graph=False, thr=0.25)),
], ids=lambda v: v if isinstance(v, str) else '-'.join('%s=%s' % kv for kv in sorted(v.items())) or 'default')
def test_shift_chain_equals_explicit_chain_other_shapes(variant, shape, kw):
    pb, _, pcfg = _setup(shape, variant, **kw)
    _shift_vs_explicit(pb, pcfg, 1, 'repeat', 'keep')
    _shift_vs_explicit(pb, pcfg, 3, 'box', 'reset', n_plans=3)


def test_shift_chain_equals_explicit_chain_stepwise():
    pb, _, pcfg = _setup('small', 'safe', thr=0.5, use_graph=False)
    _shift_vs_explicit(pb, pcfg, 1, 'box', 'keep', stepwise=True)


# ---------------------------------------------------------------------------------------------------------------- 3. against the oracle
@pytest.mark.parametrize('thr', [-1.0, 0.5])
@pytest.mark.parametrize('rule', RULES)
@pytest.mark.parametrize('tail', TAILS)
@pytest.mark.parametrize('variant', ['cem', 'safe'])
def test_warm_chain_matches_the_composed_oracle(variant, tail, rule, thr):
    """16 chains of 4 plans on explicit noise (problem seed 7, noise seeds 100 + plan, drift N(0, 0.02) from seed 5), the oracle fed by
    its OWN mu / sigma: iterations equal, elite sets equal in every iteration, |score| within 2e-5, action rtol 1e-5 / atol 1e-6 (the
    tolerances of tests/test_gpu_batch.py at this shape; the oracle's fp32 and fp64 runs agree to 2.4e-7 / 1.4e-7 over these chains).
    The elite set of an iteration is read back after a stepwise select."""
    pb, ocfg, pcfg = _setup('small', variant, thr=thr, use_graph=False)
    N, H, P, I = SMALL['N'], SMALL['H'], SMALL['P'], SMALL['I']
    pl = hp.make_planner(pb, pcfg)
    pl.set_warm_start(shift=1, tail=tail, sigma=rule, floor_frac=0.25)
    pl.set_init_mode('shift')
    mu0, sg0 = wc.box(pb, H)
    fl = _floor(pcfg)
    omu = osg = None
    for p, st in enumerate(_states(pb, 4)):
        eps = hp.noise(I, N, H, 2, P, 60, seed=100 + p)
        m, g = (mu0, sg0) if omu is None else wc.shift(omu, osg, mu0[0], sg0[0], 1, TAILS.index(tail), RULES.index(rule), fl)
        ra, rs, rit, omu, osg, rel = wc.oracle_plan(st, pb, ocfg, eps, m, g)
        pl.plan_begin(st, eps_act=eps[0], eps_model=eps[1])
        elites = []
        for it in range(I):
            pl.plan_rollout(it)
            pl.plan_select(it)
            if it < rit:
                elites.append(np.sort(pl.elite_idx().cpu().numpy()))
        a, sc, it_run = pl.plan_end(eps_out=eps[2])
        print('%s %s %s thr %g plan %d: iters %d/%d dscore %.2e dact %.2e' % (variant, tail, rule, thr, p, it_run, rit, abs(sc - rs), np.max(np.abs(a - ra))))
        assert it_run == rit, (p, it_run, rit)
        for it in range(rit):
            np.testing.assert_array_equal(elites[it], rel[it], err_msg='plan %d iteration %d elite set' % (p, it))
        assert abs(sc - rs) <= 2e-5, (p, sc, rs)
        assert np.allclose(a, ra, rtol=1e-5, atol=1e-6), (p, a, ra)
    pl.close()


# ---------------------------------------------------------------------------------------------------------------- 4. batch
def _batch(pb, pcfg, mb):
    from ethz_safe_learning_amd import BatchCemPlanner
    pl = BatchCemPlanner(pcfg, mb)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


@pytest.mark.parametrize('variant,shape,thr', [('cem', 'small', 0.5), ('safe', 'small', -1.0), ('cem', 'cem_mpc', 0.25), ('safe', 'safe_cem_mpc', 0.25)])
def test_batched_chain_with_a_moving_slot_map_equals_the_single_chains(variant, shape, thr):
    """Six environments (slots) on a batch handle of 8, each mirrored by a single-state handle of its own.  The calls vary n_states,
    permute the slot map, reset slot 2 mid-chain and leave slot 4 out for two calls; every problem must equal its slot's single plan
    bit for bit, the graph is captured once, and the launches per iteration are a cold batch handle's."""
    pb, _, pcfg = _setup(shape, variant, thr=thr)
    bp, cold = _batch(pb, pcfg, 8), _batch(pb, pcfg, 8)
    bp.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
    bp.set_init_mode('shift', slot=None)
    singles = []
    for e in range(6):
        sp = hp.make_planner(pb, pcfg)
        sp.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
        sp.set_init_mode('shift')
        singles.append(sp)
    walks = [_states(pb, 8, seed=40 + e) for e in range(6)]
    steps = [0] * 6
    schedule = [                                             # (slots of the call, slot to reset first)
        ([0, 1, 2, 3, 4, 5], None),
        ([5, 3, 1, 0, 2, 4], None),                          # (b) a permutation
        ([2, 0, 5], None),                                   # (a) fewer problems, (d) 4 sits out ...
        ([1, 2, 3, 0, 5], 2),                                # (c) slot 2 restarts; 4 still out
        ([4, 0, 1], None),                                   # ... and comes back in front, its carry two calls old
        ([3, 4, 5, 2, 1, 0], None),
    ]
    cold.plan_batch(np.stack([walks[e][0] for e in range(6)]), seed=2, calls=np.arange(6, dtype=np.uint64))
    for c, (slots, rst) in enumerate(schedule):
        if rst is not None:
            bp.reset_carry(rst)
            singles[rst].reset_carry()
        states = np.stack([walks[e][steps[e]] for e in slots])
        calls = np.array([100 * e + steps[e] for e in slots], np.uint64)
        acts, scores, iters = bp.plan_batch(states, seed=2, calls=calls, slots=slots)
        for b, e in enumerate(slots):
            a1, s1, i1 = singles[e].plan(states[b], seed=2, call=int(calls[b]))
            np.testing.assert_array_equal(acts[b], a1, err_msg='call %d slot %d action' % (c, e))
            assert scores[b] == np.float32(s1) and iters[b] == i1, (c, e, scores[b], s1, iters[b], i1)
            mb_, sb_, vb = bp.carry(e)
            m1, g1, v1 = singles[e].carry()
            assert vb and v1
            np.testing.assert_array_equal(mb_, m1, err_msg='call %d slot %d carried mu' % (c, e))
            np.testing.assert_array_equal(sb_, g1, err_msg='call %d slot %d carried sigma' % (c, e))
            steps[e] += 1
        for e in set(range(6)) - set(slots):                 # a slot that sat the call out keeps its carry
            mb_, sb_, vb = bp.carry(e)
            m1, g1, v1 = singles[e].carry()
            assert vb == v1
            np.testing.assert_array_equal(mb_, m1)
            np.testing.assert_array_equal(sb_, g1)
        assert bp.graph_status() == 'graph'
    assert bp.launches_per_iteration() == cold.launches_per_iteration()
    with pytest.raises(Exception):
        bp.set_carry_slots([0, 0, 1])                         # not distinct
    with pytest.raises(Exception):
        bp.set_carry_slots([0, 8])                            # out of range
    for p in singles + [bp, cold]:
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 5. invalidation, errors
def test_first_shift_plan_and_plan_after_reset_are_cold():
    pb, _, pcfg = _setup('small', 'cem', thr=0.5)
    plain, warm = hp.make_planner(pb, pcfg), hp.make_planner(pb, pcfg)
    warm.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
    warm.set_init_mode('shift')
    assert warm.carry()[2] is False
    sts = _states(pb, 3)
    _same(_snapshot(warm, warm.plan(sts[0], seed=4, call=0)), _snapshot(plain, plain.plan(sts[0], seed=4, call=0)), 'first shift plan')
    w1 = _snapshot(warm, warm.plan(sts[1], seed=4, call=1))
    c1 = _snapshot(plain, plain.plan(sts[1], seed=4, call=1))
    assert not np.array_equal(w1['musig'], c1['musig'])                       # the second plan really was warm
    warm.reset_carry()
    assert warm.carry()[2] is False
    _same(_snapshot(warm, warm.plan(sts[2], seed=4, call=2)), _snapshot(plain, plain.plan(sts[2], seed=4, call=2)), 'after reset_carry')
    assert warm.carry()[2] is True
    # set_weights / set_normaliser keep the carry
    warm.set_weights(pb['weights'])
    warm.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    m, g, v = warm.carry()
    assert v
    np.testing.assert_array_equal(np.stack([m, g]), warm.mu_sigma().cpu().numpy())
    plain.close()
    warm.close()


def test_bad_arguments_leave_the_handle_usable():
    from ethz_safe_learning_amd import _capi
    pb, _, pcfg = _setup('small', 'cem')
    pl = hp.make_planner(pb, pcfg)
    H, A = pcfg.horizon, pcfg.act_dim
    mu0, sg0 = wc.box(pb, H)

    def status(fn, *a, **k):
        with pytest.raises(_capi.CemError) as e:
            fn(*a, **k)
        return e.value.status

    assert status(pl.set_warm_start, shift=0) == 1 and status(pl.set_warm_start, shift=H) == 1
    assert status(pl.set_warm_start, sigma='keep', floor_frac=-0.1) == 1 and status(pl.set_warm_start, sigma='keep', floor_frac=float('inf')) == 1
    assert status(pl.set_init_mode, 3) == 1 and status(pl.set_init_mode, 'cold', slot=1) == 1
    bad = sg0.copy(); bad[2, 1] = -1e-3
    assert status(pl.set_initial_distribution, mu0, bad) == 1
    bad = mu0.copy(); bad[0, 0] = np.nan
    assert status(pl.set_initial_distribution, bad, sg0) == 1
    bad = sg0.copy(); bad[H - 1, A - 1] = np.inf
    assert status(pl.set_initial_distribution, mu0, bad) == 1
    assert status(pl.carry, 1) == 1 and status(pl.reset_carry, 1) == 1
    ws = _capi.CemWarmStart(shift=1, tail=2)
    assert pl.lib.cem_planner_set_warm_start(pl.h, ws) == 1
    assert pl.lib.cem_planner_set_carry_slots(pl.h, 1, None) == 7             # a single-state handle has no slot map
    pl.set_init_mode('explicit')
    assert status(pl.plan, pb['state'], seed=1, call=0) == 7                   # EXPLICIT without an upload: CEM_ERR_STATE
    assert pl.carry()[2] is False
    pl.set_init_mode('cold')
    plain = hp.make_planner(pb, pcfg)
    _same(_snapshot(pl, pl.plan(pb['state'], seed=1, call=0)), _snapshot(plain, plain.plan(pb['state'], seed=1, call=0)), 'after the refusals')
    pl.close()
    plain.close()


def test_shift_after_a_recovered_fused_select_carries_what_select_mode_2_carries():
    pb, _, pcfg3 = _setup('B2', 'cem', select_mode=3)
    _, _, pcfg2 = _setup('B2', 'cem', select_mode=2)
    f, m2 = hp.make_planner(pb, pcfg3), hp.make_planner(pb, pcfg2)
    for pl in (f, m2):
        pl.set_warm_start(shift=1, tail='box', sigma='keep', floor_frac=0.25)
        pl.set_init_mode('shift')
    sts = _states(pb, 3)
    f.plan(sts[0], seed=6, call=0)
    m2.plan(sts[0], seed=6, call=0)
    assert f.select_mode() == 3
    f.inject_fault(1)
    r = f.plan(sts[1], seed=6, call=1)                                       # recovered in stream: CEM_OK, select_mode 2 from now on
    assert f.select_mode() == 2
    r2 = m2.plan(sts[1], seed=6, call=1)
    cf, c2 = f.carry(), m2.carry()
    assert cf[2] and c2[2]
    np.testing.assert_array_equal(r[0], r2[0])                                # the recovered plan has select_mode 2's bits ...
    assert np.float32(r[1]) == np.float32(r2[1]) and r[2] == r2[2], (r, r2)
    np.testing.assert_array_equal(cf[0], c2[0])                              # ... and so has what it carries
    np.testing.assert_array_equal(cf[1], c2[1])
    # and the next plan is a warm one from that carry: equal to an EXPLICIT plan fed with its shift
    ref = hp.make_planner(pb, pcfg2)
    mu0, sg0 = wc.box(pb, pcfg2.horizon)
    ref.set_initial_distribution(*wc.shift(cf[0], cf[1], mu0[0], sg0[0], 1, 0, 1, _floor(pcfg2)))
    ref.set_init_mode('explicit')
    _same(_snapshot(f, f.plan(sts[2], seed=6, call=2)), _snapshot(ref, ref.plan(sts[2], seed=6, call=2)), 'plan after the recovery')
    for p in (f, m2, ref):
        p.close()


# ---------------------------------------------------------------------------------------------------------------- 6. policy layer
def _warm_policy(seed=11, **kw):
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    env, model, _ = make_agent_parts('cem_mpc', seed=seed)
    trained_like(model, np.random.default_rng(seed))
    return env, model, CemMpc(model=model, environment=env, **dict(POLICIES_YAML['cem_mpc'], **kw))


def _obs(n, seed=3):
    rng = np.random.default_rng(seed)
    st = np.zeros(60, np.float32); st[3:19] = 0.5; st[22:38] = 0.6
    return [st + rng.normal(0, 0.02, 60).astype(np.float32) * i for i in range(n)]


def _planner_like(pol, model):
    from ethz_safe_learning_amd import CemPlanner
    pl = CemPlanner(pol.planner_config())
    pl.set_weights(model.model.get_weights())
    pl.set_normaliser(model.inputs_min, model.inputs_max)
    return pl


def test_policy_chain_equals_the_planner_chain_and_policies_do_not_share_a_carry():
    kw = dict(warm_start=True, warm_shift=1, warm_tail='repeat', warm_sigma='keep', warm_sigma_floor=0.25)
    env, model, pol = _warm_policy(**kw)
    ref = _planner_like(pol, model)
    ref.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
    ref.set_init_mode('shift')
    cold = _planner_like(pol, model)
    obs = _obs(4)
    for i, ob in enumerate(obs[:3]):
        np.testing.assert_array_equal(pol.generate_action(ob), ref.plan(ob, seed=pol.seed, call=i)[0], err_msg='decision %d' % i)
        cold.plan(ob, seed=pol.seed, call=i)
    # a second warm policy of the same shape on the same model: its first plan is cold although the first policy has a carry
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from tests.test_simba_api import POLICIES_YAML
    pol2 = CemMpc(model=model, environment=env, **dict(POLICIES_YAML['cem_mpc'], **kw))
    a2 = pol2.generate_action(obs[0])
    assert pol2._planner is not pol._planner
    fresh = _planner_like(pol, model)
    np.testing.assert_array_equal(a2, fresh.plan(obs[0], seed=pol.seed, call=0)[0])
    assert pol._planner.carry()[2] and not np.array_equal(pol._planner.carry()[0], pol2._planner.carry()[0])
    # ... and the first policy's chain went on undisturbed
    np.testing.assert_array_equal(pol.generate_action(obs[3]), ref.plan(obs[3], seed=pol.seed, call=3)[0])
    # reset(): the next plan has the cold plan's bits
    pol.reset()
    assert not pol._planner.carry()[2]
    np.testing.assert_array_equal(pol.generate_action(obs[1]), cold.plan(obs[1], seed=pol.seed, call=4)[0])
    # a policy without warm start shares the shape's handle as before and ignores reset()
    _, _, p3 = _warm_policy()
    _, _, p4 = _warm_policy()
    p3.reset()
    p3.generate_action(obs[0]); p4.generate_action(obs[0])
    assert p3._planner is p4._planner


def test_generate_actions_with_slots_and_reset_equals_per_environment_chains():
    """Three environments on one warm policy; rows are compacted and reordered between decisions, environment 1 restarts once.  Row b
    must be what a single-state warm chain of ITS environment returns with the environment's own call number (e * 2**32 + decision)."""
    kw = dict(warm_start=True, warm_shift=1, warm_tail='box', warm_sigma='keep', warm_sigma_floor=0.25)
    env, model, pol = _warm_policy(**kw)
    chains = []
    for e in range(3):
        pl = _planner_like(pol, model)
        pl.set_warm_start(shift=1, tail='box', sigma='keep', floor_frac=0.25)
        pl.set_init_mode('shift')
        chains.append(pl)
    obs = [_obs(6, seed=20 + e) for e in range(3)]
    t = [0, 0, 0]
    for slots, reset in (([0, 1, 2], [True, True, True]), ([0, 1, 2], None), ([2, 0], [False, False]), ([1, 2, 0], [True, False, False]), ([1], None)):
        st = np.stack([obs[e][t[e]] for e in slots])
        acts = pol.generate_actions(st, slots=slots, reset=reset)
        for b, e in enumerate(slots):
            if reset is not None and reset[b]:
                chains[e].reset_carry()
            np.testing.assert_array_equal(acts[b], chains[e].plan(st[b], seed=pol.seed, call=(e << 32) + t[e])[0], err_msg='slots %s row %d' % (slots, b))
            t[e] += 1
    assert len(pol._batch_planners) == 1                      # one handle held every environment's carry throughout


def _records_equal(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if k == 'info':
            assert [sorted(i.items()) for i in a[k]] == [sorted(i.items()) for i in b[k]], (what, k)
        else:
            np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg='%s: %s' % (what, k))


def test_lockstep_on_four_environments_equals_four_sample_trajectory_runs():
    """The real agent and the real warm-started policy: four Point-Goal environments with episode lengths 3, 5, 4, 6 sampled in lockstep
    (batch_size 14: environment 0 ends first and starts a second episode while the others go on; later the rows compact to [0, 1, 3] and
    [0, 3]) against the same four environments sampled one after the other with sample_trajectory, each by a policy of its own whose
    `slot` is the environment's index.  Every record (observations, actions, rewards, ...) must be equal: the chain agent ->
    generate_actions(slots, reset) -> batch handle -> carry per slot gives every environment the plans it gets alone."""
    from ethz_safe_learning_amd.simba.agents.agent import BaseAgent
    from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from tests.test_simba_api import POLICIES_YAML
    kw = dict(POLICIES_YAML['cem_mpc'], warm_start=True, warm_tail='repeat', warm_sigma='keep', warm_sigma_floor=0.25)
    _, model, _ = _warm_policy()
    lengths = [3, 5, 4, 6]
    envs = lambda: [PointGoalEnv(num_steps=n, seed=50 + e) for e, n in enumerate(lengths)]
    agent = BaseAgent(replay_buffer_size=1000, add_observation_noise=False, action_repeat=1)

    es = envs()
    pol = CemMpc(model=model, environment=es[0], **kw)
    paths, steps = agent.sample_trajectories_lockstep(es, pol, batch_size=14, max_trajectory_length=100)
    assert steps == 3 + 5 + 4 + 6 + 3 and len(paths) == 5        # environment 0 ran two episodes
    assert len(pol._batch_planners) == 1 and 4 in pol._batch_planners

    es = envs()
    want = []
    for e, n_ep in enumerate([2, 1, 1, 1]):
        pe = CemMpc(model=model, environment=es[e], **kw)
        pe.slot = e
        for _ in range(n_ep):
            want.append(agent.sample_trajectory(es[e], pe, max_trajectory_length=100)[0])
    assert len(want) == len(paths)
    for i, (a, b) in enumerate(zip(paths, want)):
        _records_equal(a, b, 'record %d' % i)


def test_a_plan_staged_twice_hands_its_carry_over_once():
    """A plan whose graph capture is refused (what a communicator meets on a stack without captured collectives; injected here) is staged
    for the capture and again for the eager launches that replace it.  The pending carry must reach that plan's first kernel all the
    same: the chain equals a kernel-by-kernel handle's, plan after plan."""
    pb, _, pcfg_g = _setup('small', 'safe', thr=0.5, use_graph=True)
    _, _, pcfg_e = _setup('small', 'safe', thr=0.5, use_graph=False)
    g, e = hp.make_planner(pb, pcfg_g), hp.make_planner(pb, pcfg_e)
    for pl in (g, e):
        pl.set_warm_start(shift=1, tail='repeat', sigma='keep', floor_frac=0.25)
        pl.set_init_mode('shift')
    sts = _states(pb, 4)
    eps = hp.noise(SMALL['I'], SMALL['N'], SMALL['H'], 2, SMALL['P'], 60, seed=9)
    for pl in (g, e):                                         # plan 0 on explicit noise: never captured, leaves a carry
        pl.plan(sts[0], eps_act=eps[0], eps_model=eps[1], eps_out=eps[2])
    assert g.graph_status() == 'eager'
    g.inject_fault(2)
    for i in (1, 2, 3):                                       # plan 1: capture attempted, refused, staged again, launched eagerly
        _same(_snapshot(g, g.plan(sts[i], seed=8, call=i)), _snapshot(e, e.plan(sts[i], seed=8, call=i)), 'plan %d' % i)
        np.testing.assert_array_equal(g.carry()[0], e.carry()[0])
        assert g.graph_status() == 'graph-unsupported'
    g.close()
    e.close()
