"""Batched planning swept over random shapes (tests/batch_cases.py) on the MI355X.  tests/test_gpu_batch.py holds the batch path to
single plans at the shipped shapes (obs 60, act 2, units 128); at A = 2 several wrong per-problem strides give the right address, so
these cases sweep what the slice addressing depends on — action dims 1 .. 12, obs + act on both sides of 64, narrow and odd widths,
members that split a particle, every tile size, forced segments on the single side, both samplers, graph and eager, early stop — with:
  * every problem of a batch bit for bit equal to its single-state plan (action, best score, iterations), n_states replayed;
  * first-iteration slices of every problem (actions, scores, elite set, mu / sigma, returned action) against the fp64 oracle;
  * isolation: a problem's inputs reach its own outputs only, equal inputs give equal outputs, and a plan of fewer problems leaves
    the rest of the workspace's problems alone;
  * BASELINE B1 and B4 (three action quads, two input blocks per wave), and a full batch of CEM_MAX_BATCH problems.
A failure prints the case dict; the generator seed reproduces it."""
import os

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import batch_cases as bc
from tests import helpers as hp
from tests.test_gpu_parity import ATOL

pytestmark = pytest.mark.gpu
# CEM_FUZZ_SCALE=n multiplies the number of seeds (as tests/test_gpu_fuzz.py does)
SCALE = int(os.environ.get('CEM_FUZZ_SCALE', '1'))


def _sampler(monkeypatch, which):
    """CEM_FORCE_SAMPLER ('tile' | 'kernel') for the handles created next, or None: the automatic rule."""
    if which:
        monkeypatch.setenv('CEM_FORCE_SAMPLER', which)
    else:
        monkeypatch.delenv('CEM_FORCE_SAMPLER', raising=False)


def _batch(pb, pcfg, max_batch):
    from ethz_safe_learning_amd import BatchCemPlanner
    pl = BatchCemPlanner(pcfg, max_batch)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


def _singles(single, states, seed, calls, which=None):
    which = range(len(states)) if which is None else which
    out = [single.plan(states[b], seed=seed, call=int(calls[b])) for b in which]
    return (np.stack([a for a, _, _ in out]), np.array([s for _, s, _ in out], np.float32), np.array([i for _, _, i in out], np.int32))


def _assert_same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg='%s: actions' % what)
    np.testing.assert_array_equal(got[1], want[1], err_msg='%s: scores' % what)
    np.testing.assert_array_equal(got[2], want[2], err_msg='%s: iterations' % what)


def _slices(pl, c, mb):
    """Copies of every problem's per-problem workspace arrays: {name: [mb, ...]}."""
    import torch
    N, H, A, P, k = c['N'], c['H'], c['A'], c['P'], c['k']
    lay = pl.layout
    pl.synchronize()
    out = dict(scores=pl._view(lay.scores_local, mb * N, torch.float32).view(mb, N),
               elite=pl._view(lay.elite_idx, mb * k, torch.int32).view(mb, k),
               musig=pl._view(lay.mu_sigma, mb * 2 * H * A, torch.float32).view(mb, 2, H, A),
               actions=pl._view(lay.actions, mb * N * H * A, torch.float32).view(mb, N, H, A),
               returns=pl._view(lay.returns, mb * P * N, torch.float32).view(mb, P, N))
    if c['variant'] == 'safe':
        out['costs'] = pl._view(lay.costs, mb * H * P * N, torch.uint8).view(mb, H, P, N)
    return {name: v.cpu().numpy().copy() for name, v in out.items()}


# ------------------------------------------------------------------------------------------------------------ batch vs single plans
@pytest.mark.parametrize('seed', range(bc.N_CASES * SCALE))
def test_random_batch_problems_equal_their_single_plans(seed, monkeypatch):
    c = bc.random_batch_case(seed)
    _sampler(monkeypatch, c['sampler'])
    pb = bc.problem(c)
    _, pcfg = bc.configs(pb, c)
    single = hp.make_planner(pb, pcfg)
    mb = c['max_batch']
    pl = _batch(pb, pcfg, mb)
    plan_seed = (1 << 33) + 17 * seed                  # (the seed's high word too)
    # the case's n_states, then a replay of the same handle (the same captured graph) with another
    n2 = mb if c['n_states'] < mb else max(1, mb // 2)
    for rnd, n in enumerate((c['n_states'], n2)):
        states = bc.states(pb, n, seed=1000 * seed + rnd)
        calls = bc.calls(n, seed=2000 * seed + rnd)
        got = pl.plan_batch(states, seed=plan_seed, calls=calls)
        _assert_same(got, _singles(single, states, plan_seed, calls), '%s, n_states %d' % (c, n))
        assert np.all(got[2] >= 1) and np.all(got[2] <= c['I']), c
        if c['use_graph']:
            assert pl.graph_status() == 'graph', c
    pl.close()
    single.close()


# ------------------------------------------------------------------------------------------------------------ batch vs the oracle
@pytest.mark.parametrize('seed', range(bc.N_ORACLE_CASES * SCALE))
def test_random_batch_problems_match_the_oracle_in_the_first_iteration(seed, monkeypatch):
    """I = 1 on explicit noise with a leading problem axis.  Each problem's slices: the sampled actions (bit-exact), every candidate's
    score (fp64, proven threshold crossings admitted), the elite set and mu / sigma (the oracle's select on the GPU's own scores, and the
    elite set against the oracle's scores modulo ties), and the returned action — the one reader of the problem's eps_out slice."""
    c = bc.random_batch_case(seed, oracle=True)
    _sampler(monkeypatch, c['sampler'])
    pb = bc.problem(c)
    ocfg, pcfg = bc.configs(pb, c)
    O, A, N, H, P, k, n = c['O'], c['A'], c['N'], c['H'], c['P'], c['k'], c['n_states']
    pl = _batch(pb, pcfg, c['max_batch'])
    states = bc.states(pb, n, seed=seed)
    ns = [hp.noise(1, N, H, A, P, O, seed=100 * seed + b) for b in range(n)]
    ea, em, eo = (np.stack([x[i] for x in ns]) for i in range(3))
    acts, scores, iters = pl.plan_batch(states, calls=np.zeros(n, np.uint64), eps_act=ea, eps_model=em, eps_out=eo)
    sl = _slices(pl, c, c['max_batch'])
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    mu_0, sg_0 = np.broadcast_to(mu0, (H, A)).astype(np.float32), np.broadcast_to(sg0, (H, A)).astype(np.float32)
    w64 = o.cast_weights(pb['weights'], np.float64)
    sp = pb['scorer']
    amag = max(1.0, float(np.abs(ub).max()))
    for b in range(n):
        what = '%s, problem %d' % (c, b)
        actions, sc, el = sl['actions'][b], sl['scores'][b], np.sort(sl['elite'][b])
        ref_actions = o.sample_actions(mu_0, sg_0, lb, ub, ea[b, 0])
        np.testing.assert_array_equal(actions, ref_actions, err_msg=what)
        ref64, traj64 = o.candidate_scores(states[b].astype(np.float64), ref_actions.astype(np.float64), w64, pb['inputs_min'],
                                           pb['inputs_max'], em[b, 0], ocfg, sp, return_traj=True)
        _, _, flipped = hp.assert_scores_match_oracle(sc, traj64, P, N, sp, c['variant'], c['post'], ATOL, what)
        # the select and refit on the GPU's own scores: exact elite set (ties to the lower index), mu / sigma, best, the action
        mu, sigma, best, best_score, ref_elite, _ = o.select_and_refit(sc, actions, mu_0, sg_0, np.zeros(A, np.float32),
                                                                        np.float32(-np.inf), ocfg)
        np.testing.assert_array_equal(el, ref_elite, err_msg=what)
        if not flipped:
            assert hp.elite_sets_equal_modulo_ties(ref64, el, o.top_k(ref64, k), 2e-5), what
        np.testing.assert_allclose(sl['musig'][b, 0], mu, rtol=1e-5, atol=1e-6 * amag, err_msg=what)
        sig_atol = 1e-6 * amag + 4 * 1.2e-7 * float(np.abs(mu).max()) * np.sqrt(k)      # (test_gpu_fuzz.py: one-point Box dimensions)
        np.testing.assert_allclose(sl['musig'][b, 1], sigma, rtol=2e-5, atol=sig_atol, err_msg=what)
        assert iters[b] == 1, what
        np.testing.assert_array_equal(acts[b], best + eo[b] * np.float32(c['noise']), err_msg=what)
        assert scores[b] == best_score, (what, scores[b], best_score)
        # the whole (one-iteration) plan of the oracle on the same slices, where its fp32 select picks the same elite set
        trace = []
        ra, rs, rit = o.do_generate_action(states[b], pb['weights'], pb['inputs_min'], pb['inputs_max'], pb['low'], pb['high'],
                                           ea[b], em[b], eo[b], ocfg, sp, trace=trace)
        assert rit == 1, what
        if np.array_equal(el, np.sort(trace[0]['elite'])):
            np.testing.assert_allclose(acts[b], ra, rtol=1e-5, atol=1e-6 * amag, err_msg=what)
            assert abs(scores[b] - rs) <= 2e-5 + 6e-8 * abs(rs), (what, scores[b], rs)
    pl.close()


# ------------------------------------------------------------------------------------------------------------ isolation and the tail
@pytest.mark.parametrize('seed', bc.isolation_seeds())
def test_problems_are_isolated_and_the_tail_is_untouched(seed, monkeypatch):
    """At a full batch (n_states = max_batch, at least three iterations so that mu / sigma are refitted):
    leave-one-out — problem j's new state and call change problem j's outputs and no other problem's (results and workspace slices);
    duplicates — two slots with the same (state, call) return the same bits; the tail — a plan of n < max_batch problems leaves the
    slices of problems n .. max_batch - 1 as they were, bit for bit, except mu / sigma, which the plan's first kernel restarts for
    every problem of the handle (cem_init_kernel: the initial distribution, exactly)."""
    c = dict(bc.random_batch_case(seed))
    c['I'] = max(c['I'], 3)
    _sampler(monkeypatch, c['sampler'])
    pb = bc.problem(c)
    _, pcfg = bc.configs(pb, c)
    mb = c['max_batch']
    pl = _batch(pb, pcfg, mb)
    plan_seed = 5 + seed
    states, calls = bc.states(pb, mb, seed=seed), bc.calls(mb, seed=seed)
    base = pl.plan_batch(states, seed=plan_seed, calls=calls)
    s0 = _slices(pl, c, mb)
    # leave-one-out
    j = mb // 2
    st2, cl2 = states.copy(), calls.copy()
    st2[j] += np.random.default_rng(seed).normal(0.0, 0.1, st2[j].shape).astype(np.float32)
    cl2[j] = calls.max() + np.uint64(1)
    got = pl.plan_batch(st2, seed=plan_seed, calls=cl2)
    s1 = _slices(pl, c, mb)
    others = np.array([b for b in range(mb) if b != j])
    _assert_same(tuple(x[others] for x in got), tuple(x[others] for x in base), '%s, leave-one-out j=%d' % (c, j))
    for name in s0:
        np.testing.assert_array_equal(s1[name][others], s0[name][others], err_msg='%s, leave-one-out j=%d: %s' % (c, j, name))
    assert not (np.array_equal(got[0][j], base[0][j]) and got[1][j] == base[1][j]), (c, 'problem j did not change')
    # duplicates: slot mb - 1 repeats slot 0
    st3, cl3 = states.copy(), calls.copy()
    st3[mb - 1], cl3[mb - 1] = st3[0], cl3[0]
    got = pl.plan_batch(st3, seed=plan_seed, calls=cl3)
    s3 = _slices(pl, c, mb)
    _assert_same(tuple(x[mb - 1] for x in got), tuple(x[0] for x in got), '%s, duplicates' % c)
    _assert_same(tuple(x[:mb - 1] for x in got), tuple(x[:mb - 1] for x in base), '%s, duplicates (the other slots)' % c)
    for name in s3:
        np.testing.assert_array_equal(s3[name][mb - 1], s3[name][0], err_msg='%s, duplicates: %s' % (c, name))
    # the tail: fewer problems, other states and calls
    n = max(1, mb // 2)
    got = pl.plan_batch(bc.states(pb, n, seed=seed + 1) + np.float32(0.01), seed=plan_seed + 1, calls=bc.calls(n, seed=seed + 1))
    s4 = _slices(pl, c, mb)
    for name in s3:
        if name != 'musig':
            np.testing.assert_array_equal(s4[name][n:], s3[name][n:], err_msg='%s, tail after n_states %d: %s' % (c, n, name))
    _, _, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    np.testing.assert_array_equal(s4['musig'][n:, 0], np.broadcast_to(mu0, (mb - n, c['H'], c['A'])), err_msg='%s, tail mu' % c)
    np.testing.assert_array_equal(s4['musig'][n:, 1], np.broadcast_to(sg0, (mb - n, c['H'], c['A'])), err_msg='%s, tail sigma' % c)
    assert not np.array_equal(s4['scores'][:n], s3['scores'][:n]), c                  # (the head did plan again)
    pl.close()


# ------------------------------------------------------------------------------------------------------------ B1, B4, a full batch
# BASELINE B1 and B4 (tests/test_batch_capi_cpu.py SHAPES) with fewer iterations: B4 is obs 100, act 12 (three action quads, two input
# blocks per wave), 32 768 rows of 50 steps per problem
BIG = {
    'B1': dict(O=60, A=2, E=5, P=5, N=500, H=25, k=50, I=3),
    'B4': dict(O=100, A=12, E=8, P=8, N=4096, H=50, k=409, I=2),
}


@pytest.mark.parametrize('use_graph', [True, False])
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('shape', sorted(BIG))
def test_baseline_shapes_batch_equals_single_plans(shape, variant, use_graph, monkeypatch):
    _sampler(monkeypatch, None)
    s = BIG[shape]
    pb = hp.make_problem(s['O'], s['A'], s['E'], 4, seed=1234)
    _, pcfg = hp.configs(pb, N=s['N'], H=s['H'], P=s['P'], E=s['E'], k=s['k'], I=s['I'], variant=variant, noise=1e-3, post=0.2,
                         use_graph=use_graph)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, 3)
    states, calls = bc.states(pb, 3, seed=3), bc.calls(3, seed=4)
    got = pl.plan_batch(states, seed=21, calls=calls)
    _assert_same(got, _singles(single, states, 21, calls), '%s %s graph=%s' % (shape, variant, use_graph))
    assert len({tuple(a) for a in got[0]}) == 3
    if use_graph:
        assert pl.graph_status() == 'graph'
    pl.close()
    single.close()


def test_a_full_batch_at_the_shipped_cem_shape(monkeypatch):
    """CEM_MAX_BATCH problems at the shipped cem_mpc shape, the automatic sampler rule: 256 problems' tiles cannot all be resident, so
    the rule moves the sampler into a launch of its own — one launch per iteration more than the 8-problem handle, whose tiles all fit.
    A spread of problems against single plans, then the same handle with 255 problems."""
    _sampler(monkeypatch, None)
    cap = 256
    pb = hp.make_problem(60, 2, 15, 4, seed=1234)
    _, pcfg = hp.configs(pb, N=150, H=8, P=5, E=15, k=15, I=10, variant='cem', thr=0.25, noise=1e-3, post=0.2, use_graph=True)
    single = hp.make_planner(pb, pcfg)
    pl = _batch(pb, pcfg, cap)
    small = _batch(pb, pcfg, 8)
    lpi, lpi8 = pl.launches_per_iteration(), small.launches_per_iteration()
    assert lpi == lpi8 + 1, ('256 problems: %d launches per iteration, 8 problems: %d' % (lpi, lpi8))
    small.close()
    for n, which in ((cap, [0, 1, 127, 254, 255]), (cap - 1, [0, 1, 127, 253, 254])):
        states, calls = bc.states(pb, n, seed=n), bc.calls(n, seed=n)
        got = pl.plan_batch(states, seed=3, calls=calls)
        assert got[0].shape == (n, 2) and np.all(np.isfinite(got[0])) and np.all(got[2] >= 1)
        _assert_same(tuple(x[which] for x in got), _singles(single, states, 3, calls, which), 'n_states %d' % n)
        assert pl.graph_status() == 'graph'
    pl.close()
    single.close()
