"""The ranked form of the one-workgroup select (csrc/cem_select_ranked.hip, select_form 1) against the form it stands in for
(cem_select_kernel<true, false>, form 0, kept by CEM_FORCE_SELECT=bucket at create): bit for bit in everything a select writes.

  cases   every vector of tests/select_cases.py with N <= 4096 on a CemMpc handle, on test_gpu_select_paths.py's harness (H = 3, A = 2,
          P = 5, smoothing 0.25, the vector written into the score buffer), once per form
  edges   whole plans on their own scores: N = 16 with k = 1, k = N, N = 1000, N = 4096 (form 1) and 4097 (form 0), HA = 6 and 60 (narrow
          moments), HA = 8 with k = 300 (narrow too, by the kernel's rule) and two shapes that do take the float4 moments (HA = 8 with
          k = 2100, HA = 60 with k = 200), P = 1 and P = 9 (the second batch of particle loads), a batch handle of three
          problems, and a two-iteration plan whose early stop fires in iteration 0 (the second select leaves on `done`)
  graph   one captured handle at N = 2000, k = 200, H = 30: two plans under each form

Everything is compared as uint32 views with assert_array_equal."""
import numpy as np
import pytest

from tests import helpers as hp
from tests import select_cases as sc

pytestmark = pytest.mark.gpu

H, A, P, E, SMOOTHING = 3, 2, 5, 5, 0.25
F, U = np.float32, np.uint32
CASES = [c for c in sc.CASES if c.N <= 4096]

_PB, _NOISE = {}, {}


def _problem(E_=E):
    if E_ not in _PB:
        _PB[E_] = hp.make_problem(seed=42, E=E_)
    return _PB[E_]


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, F)).view(U)


def _planner(monkeypatch, form, pb, pcfg, batch=0):
    """A handle whose one-workgroup select takes `form` where it is eligible (the variable is read at create)."""
    if form == 0:
        monkeypatch.setenv('CEM_FORCE_SELECT', 'bucket')
    else:
        monkeypatch.delenv('CEM_FORCE_SELECT', raising=False)
    if not batch:
        return hp.make_planner(pb, pcfg)
    from ethz_safe_learning_amd.planner import BatchCemPlanner
    pl = BatchCemPlanner(pcfg, batch)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


def _same(a, b, keys):
    for key in keys:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


# ---- the adversarial vectors ------------------------------------------------------------------------------------------

def _run_case(monkeypatch, case, form):
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    pb = _problem()
    _, pcfg = hp.configs(pb, N=case.N, H=H, P=P, E=E, k=case.k, I=1, smoothing=SMOOTHING, variant='cem')
    if case.N not in _NOISE:
        _NOISE[case.N] = hp.noise(1, case.N, H, A, P, 60, seed=1)
    ea, em, _ = _NOISE[case.N]
    pl = _planner(monkeypatch, form, pb, pcfg)
    try:
        out = dict(mode=pl.select_mode(), form=pl.select_form(0))
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        pl.plan_rollout(0)
        torch.cuda.synchronize()
        pl.scores_global().copy_(torch.from_numpy(case.scores))
        torch.cuda.synchronize()
        pl.plan_select(0)
        torch.cuda.synchronize()
        out['elite'] = pl.elite_idx().cpu().numpy().copy()          # as stored
        out['mu_sigma'] = _bits(pl.mu_sigma().cpu().numpy())
        out['scores_local'] = _bits(pl.scores_local().cpu().numpy())
        action, score, iters = pl.plan_end(eps_out=np.zeros(A, F))
        out['action'], out['score'], out['iters'] = _bits(action), _bits([score]), iters
    finally:
        pl.close()
    return out


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.name)
def test_case_is_bit_identical_under_both_forms(case, monkeypatch):
    r0, r1 = _run_case(monkeypatch, case, 0), _run_case(monkeypatch, case, 1)
    assert (r0['mode'], r0['form']) == (1, 0) and (r1['mode'], r1['form']) == (1, 1)
    _same(r0, r1, ('elite', 'mu_sigma', 'scores_local', 'action', 'score'))
    assert r0['iters'] == r1['iters'] == 1
    np.testing.assert_array_equal(np.sort(r1['elite']), sc.reference_top_k(case.scores, case.k))      # and the value-semantics answer itself
    np.testing.assert_array_equal(r1['elite'], np.sort(r1['elite']))                                     # ascending candidate order


# ---- whole plans on their own scores ----------------------------------------------------------------------------------

def _run_plan(monkeypatch, form, N, k, H_=3, P_=5, E_=5, I=1, thr=-1.0, batch=0, use_graph=False, plans=1):
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    pb = _problem(E_)
    _, pcfg = hp.configs(pb, N=N, H=H_, P=P_, E=E_, k=k, I=I, smoothing=SMOOTHING, variant='cem', thr=thr, use_graph=use_graph)
    pl = _planner(monkeypatch, form, pb, pcfg, batch)
    HA = H_ * A
    try:
        out = dict(mode=pl.select_mode(), form=pl.select_form(0))
        nb = max(batch, 1)
        for i in range(plans):
            if batch:
                states = np.stack([pb['state'] * F(1.0 + 0.1 * b) for b in range(batch)]).astype(F)
                action, score, iters = pl.plan_batch(states, seed=3, calls=np.arange(batch) + 10 * i)
            else:
                action, score, iters = pl.plan(pb['state'], seed=3, call=i)
            out['action%d' % i], out['score%d' % i], out['iters%d' % i] = _bits(action), _bits(np.atleast_1d(score)), np.atleast_1d(iters).copy()
        lay, t = pl.layout, torch
        out['elite'] = pl._view(lay.elite_idx, nb * k, t.int32).cpu().numpy().copy()
        out['mu_sigma'] = pl._view(lay.mu_sigma, nb * 2 * HA, t.int32).cpu().numpy().copy()
        out['scores_local'] = pl._view(lay.scores_local, nb * N, t.int32).cpu().numpy().copy()
        out['graph'] = pl.graph_status()
    finally:
        pl.close()
    return out


PLAN_KEYS = ('elite', 'mu_sigma', 'scores_local', 'action0', 'score0', 'iters0')
EDGES = [('N16_k1', dict(N=16, k=1)),
         ('k_is_N', dict(N=300, k=300)),
         ('N1000', dict(N=1000, k=100)),
         ('N4096', dict(N=4096, k=400)),
         ('HA6', dict(N=500, k=50, H_=3)),
         ('HA60', dict(N=500, k=50, H_=30)),
         ('HA8_k300', dict(N=1000, k=300, H_=4)),
         # the float4 moments need k > 16 x the narrow path's parts per column (HA = 8: 128 parts, k > 2048; HA = 60: 8 parts, k > 128)
         ('HA8_k2100_float4', dict(N=4096, k=2100, H_=4)),
         ('HA60_k200_float4', dict(N=1000, k=200, H_=30)),
         ('P1', dict(N=500, k=50, P_=1)),
         ('P9', dict(N=500, k=50, P_=9))]


@pytest.mark.parametrize('name,kw', EDGES, ids=[e[0] for e in EDGES])
def test_plan_edges_are_bit_identical_under_both_forms(name, kw, monkeypatch):
    r0, r1 = _run_plan(monkeypatch, 0, **kw), _run_plan(monkeypatch, 1, **kw)
    assert (r0['mode'], r0['form']) == (1, 0) and (r1['mode'], r1['form']) == (1, 1)
    _same(r0, r1, PLAN_KEYS)
    assert r1['iters0'][0] == 1
    assert np.all(np.diff(r1['elite']) > 0) and r1['elite'][0] >= 0 and r1['elite'][-1] < kw['N']


def test_population_above_4096_keeps_the_bucket_form(monkeypatch):
    r0, r1 = _run_plan(monkeypatch, 0, N=4097, k=400), _run_plan(monkeypatch, 1, N=4097, k=400)
    assert (r0['mode'], r0['form']) == (1, 0) and (r1['mode'], r1['form']) == (1, 0)
    _same(r0, r1, PLAN_KEYS)


def test_batch_handle_of_three_problems(monkeypatch):
    r0, r1 = _run_plan(monkeypatch, 0, N=500, k=50, batch=3), _run_plan(monkeypatch, 1, N=500, k=50, batch=3)
    assert (r0['mode'], r0['form']) == (1, 0) and (r1['mode'], r1['form']) == (1, 1)
    _same(r0, r1, PLAN_KEYS)
    assert r1['score0'].shape == (3,) and len(set(r1['score0'].tolist())) == 3          # three problems, three plans


def test_second_select_of_a_stopped_plan_stores_nothing(monkeypatch):
    """The early stop fires in iteration 0 (a threshold above any sigma): the second select returns on `done`.  What the plan leaves is
    what a one-iteration plan leaves — one blend of mu / sigma, one iteration counted — under either form."""
    stop0, stop1 = (_run_plan(monkeypatch, f, N=500, k=50, I=2, thr=1e9) for f in (0, 1))
    once = _run_plan(monkeypatch, 1, N=500, k=50, I=1)
    assert stop1['form'] == 1 and stop1['iters0'][0] == 1 and stop0['iters0'][0] == 1
    _same(stop0, stop1, PLAN_KEYS)
    _same(once, stop1, ('elite', 'mu_sigma', 'scores_local', 'action0', 'score0'))


def test_graph_handle_replays_the_ranked_select(monkeypatch):
    kw = dict(N=2000, k=200, H_=30, I=3, use_graph=True, plans=2)
    r0, r1 = _run_plan(monkeypatch, 0, **kw), _run_plan(monkeypatch, 1, **kw)
    assert (r0['form'], r1['form']) == (0, 1) and r0['graph'] == r1['graph'] == 'graph'
    _same(r0, r1, PLAN_KEYS + ('action1', 'score1', 'iters1'))
    assert r1['iters0'][0] == r1['iters1'][0] == 3
