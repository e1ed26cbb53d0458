"""Every path of the select on the adversarial score vectors of tests/select_cases.py (their routing is checked without a GPU in
tests/test_select_cases_cpu.py): one rollout on fixed noise makes the action tensor real, the case's vector is written straight into
the score buffer, one plan_select runs, and the elite set, the best action and score, mu and sigma are held against the
value-semantics reference (equal values tie by index, -0.0 == +0.0, NaN after everything).  The harness is test_select_edge_cases's:
H = 3, A = 2, P = 5, E = 5, one iteration; smoothing 0.25, so the blend is live.

Handles: CemMpc and SafeCemMpc on the one-workgroup kernel (the plain and the CROWDED instantiation; for N = 40 000 both are served by
the uncached kernel), SafeCemMpc on the automatic choice, CemMpc on the multi-workgroup chain and on its fused form; the cost
objective on two crowded cases (it takes the CROWDED instantiation too)."""
import dataclasses

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import helpers as hp
from tests import select_cases as sc

pytestmark = pytest.mark.gpu

H, A, P, E, SMOOTHING = 3, 2, 5, 5, 0.25
HANDLES = [('cem', 1), ('safe', 1), ('safe', 0), ('cem', 2), ('cem', 3)]
F = np.float32

_RUNS, _NOISE, _PB = {}, {}, []


def _run(name, variant, mode):
    """One select of the case on a fresh handle -> dict of what the device left (memoised: the bit-identity test reuses two runs)."""
    key = (name, variant, mode)
    if key in _RUNS:
        return _RUNS[key]
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    case = sc.BY_NAME[name]
    if not _PB:
        _PB.append(hp.make_problem(seed=42))
    pb = _PB[0]
    _, pcfg = hp.configs(pb, N=case.N, H=H, P=P, E=E, k=case.k, I=1, smoothing=SMOOTHING, variant='cem' if variant == 'cem' else 'safe',
                         select_mode=mode)
    if variant == 'cost':
        pcfg = dataclasses.replace(pcfg, variant='cost')
    if case.N not in _NOISE:
        _NOISE.clear()                                             # (one population's noise at a time: 144 MB at N = 40 000)
        _NOISE[case.N] = hp.noise(1, case.N, H, A, P, 60, seed=1)
    ea, em, _ = _NOISE[case.N]
    pl = hp.make_planner(pb, pcfg)
    try:
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        pl.plan_rollout(0)
        torch.cuda.synchronize()
        out = dict(actions=pl.actions().cpu().numpy().copy(), ms0=pl.mu_sigma().cpu().numpy().copy(), mode=pl.select_mode())
        pl.scores_global().copy_(torch.from_numpy(case.scores))
        torch.cuda.synchronize()
        pl.plan_select(0)
        torch.cuda.synchronize()
        out['elite'] = pl.elite_idx().cpu().numpy().copy()         # as stored
        out['ms1'] = pl.mu_sigma().cpu().numpy().copy()
        out['action'], out['score'], out['iters'] = pl.plan_end(eps_out=np.zeros(A, F))
    finally:
        pl.close()
    _RUNS[key] = out
    return out


def _check(name, variant, mode):
    case = sc.BY_NAME[name]
    r = _run(name, variant, mode)
    one_wg = case.N < 24000
    assert r['mode'] == (mode if mode else (1 if one_wg else 3))
    ref = sc.reference_top_k(case.scores, case.k)
    np.testing.assert_array_equal(np.sort(r['elite']), ref)
    best = sc.best_of(case.scores, ref)
    assert r['score'] == case.scores[best] and r['iters'] == 1
    np.testing.assert_array_equal(r['action'], r['actions'][best, 0])
    mean, var = o.moments(r['actions'][ref])
    s, oms = F(SMOOTHING), F(1.0 - SMOOTHING)                       # as o.select_and_refit blends (cem_mpc.py:64-65)
    np.testing.assert_allclose(r['ms1'][0], s * r['ms0'][0] + oms * mean, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(r['ms1'][1], s * r['ms0'][1] + oms * np.sqrt(var), rtol=2e-5, atol=1e-6)
    if case.nan:
        assert not np.isnan(case.scores[r['elite']]).any() and np.isfinite(r['score']) and np.isfinite(r['ms1']).all()


@pytest.mark.parametrize('variant,mode', HANDLES, ids=['%s-%d' % h for h in HANDLES])
@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_select_paths(case, variant, mode):
    _check(case.name, variant, mode)


@pytest.mark.parametrize('name', sc.COST_CASES)
def test_cost_handle_takes_the_crowded_select(name):
    """The cost objective's handle on two crowded cases: the reference's result, and bit for bit what SafeCemMpc's handle leaves —
    enqueue_select gives every objective but CemMpc's the CROWDED instantiation."""
    _check(name, 'cost', 1)
    c, s = _run(name, 'cost', 1), _run(name, 'safe', 1)
    np.testing.assert_array_equal(c['actions'], s['actions'])
    np.testing.assert_array_equal(c['elite'], s['elite'])
    np.testing.assert_array_equal(c['ms1'].view(np.uint32), s['ms1'].view(np.uint32))


@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_plain_and_crowded_instantiations_are_bit_identical(case):
    """The two instantiations share the compaction and the moments and differ only in how the k-th key is found: on the same actions
    (the same noise) the elite list AS STORED and mu / sigma are bit-identical on any scores."""
    c, s = _run(case.name, 'cem', 1), _run(case.name, 'safe', 1)
    np.testing.assert_array_equal(c['actions'], s['actions'])
    np.testing.assert_array_equal(c['ms0'].view(np.uint32), s['ms0'].view(np.uint32))
    np.testing.assert_array_equal(c['elite'], s['elite'])
    np.testing.assert_array_equal(c['ms1'].view(np.uint32), s['ms1'].view(np.uint32))
    assert c['score'] == s['score'] and np.array_equal(c['action'], s['action'])
