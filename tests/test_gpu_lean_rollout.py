"""The lean one-chunk rollout (csrc/cem_rollout_lean.hip: every action drawn in the lane that needs it, no materialised sample) against
the untouched generic kernels on the same seeded problem: BIT FOR BIT, after every iteration — per-row returns, scores, the [N][H][A]
actions, mu / sigma, the safe variant's per-step cost bytes — and the returned action, score and iteration count, kernel by kernel
(the stepwise API) and through the captured graph.  The reference is the generic path (CEM_FORCE_ROLLOUT=generic at create), never the
code under test."""
import numpy as np
import pytest

from tests import helpers as hp

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _run(monkeypatch, pb, force, want_path, steps, graph_plan=True, **kw):
    """One planner (created under CEM_FORCE_ROLLOUT=`force`, or left automatic): `steps` iterations kernel by kernel, everything an
    iteration leaves behind copied after each; then the same plan as one call (the captured graph where use_graph took)."""
    if force:
        monkeypatch.setenv('CEM_FORCE_ROLLOUT', force)
    else:
        monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    _, pcfg = hp.configs(pb, use_graph=True, **kw)
    pl = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    assert pl.rollout_path() == want_path
    safe = kw.get('variant', 'cem') == 'safe'
    out = dict(its=[], launches=pl.launches_per_iteration(), tiles=len(pl.tiles()[1]), segments=pl.segments())
    pl.plan_begin(pb['state'], seed=5, call=3)
    for it in range(steps):
        pl.plan_rollout(it)
        pl.plan_select(it)
        out['its'].append(dict(returns=pl.returns().cpu().numpy().copy(), scores=pl.scores_local().cpu().numpy().copy(),
                               actions=pl.actions().cpu().numpy().copy(), mu_sigma=pl.mu_sigma().cpu().numpy().copy(),
                               costs=pl.costs().cpu().numpy().copy() if safe else np.zeros(0, np.uint8)))
    out['end'] = pl.plan_end()
    if graph_plan:
        out['plan'] = pl.plan(pb['state'], seed=5, call=3)
        out['graph_status'] = pl.graph_status()
        out['after_plan'] = dict(returns=pl.returns().cpu().numpy().copy(), actions=pl.actions().cpu().numpy().copy(),
                                 mu_sigma=pl.mu_sigma().cpu().numpy().copy(), costs=pl.costs().cpu().numpy().copy() if safe else np.zeros(0, np.uint8))
    pl.close()
    return out


def _assert_same(ref, new):
    assert len(ref['its']) == len(new['its'])
    assert (ref['launches'], ref['tiles'], ref['segments']) == (new['launches'], new['tiles'], new['segments'])
    for it, (a, b) in enumerate(zip(ref['its'], new['its'])):
        assert np.isfinite(a['returns']).all() and np.isfinite(a['scores']).all()
        for key in ('actions', 'returns', 'costs', 'scores', 'mu_sigma'):
            np.testing.assert_array_equal(a[key], b[key], err_msg='%s after iteration %d' % (key, it))
    for key in ('end', 'plan'):
        if key in ref:
            np.testing.assert_array_equal(ref[key][0], new[key][0], err_msg=key)
            assert ref[key][1] == new[key][1] and ref[key][2] == new[key][2], key
    if 'after_plan' in ref:
        assert ref['graph_status'] == new['graph_status']
        for key in ('actions', 'returns', 'costs', 'mu_sigma'):
            np.testing.assert_array_equal(ref['after_plan'][key], new['after_plan'][key], err_msg='%s after the whole plan' % key)


def _compare(monkeypatch, pb, steps, lean=True, **kw):
    ref = _run(monkeypatch, pb, 'generic', 'generic', steps, **kw)
    new = _run(monkeypatch, pb, None, 'lean' if lean else 'generic', steps, **kw)
    _assert_same(ref, new)
    return ref, new


CASES = {
    # obs, act, E = P, N, H, I, segments, variant, sampling, lean
    'ragged_last_tile': (60, 2, 2, 40, 3, 2, 1, 'cem', True, True),                # the last tile of each member has 8 rows
    'every_tile_floats': (60, 2, 2, 40, 3, 2, 3, 'cem', True, True),               # a hand-over at every step
    'pinned_and_floating': (60, 2, 2, 2100, 4, 1, 2, 'cem', True, True),           # 264 tiles: 256 pinned + 8 floating, the B2 form
    'act_1_of_4': (12, 1, 2, 40, 3, 2, 1, 'cem', True, True),                      # partial action quad
    'act_3_of_4': (12, 3, 2, 40, 3, 2, 1, 'cem', True, True),
    'act_4_of_4': (12, 4, 2, 40, 3, 2, 1, 'cem', True, True),                      # full action quad
    'two_action_quads': (56, 6, 2, 40, 3, 2, 1, 'cem', True, True),
    'safe_cost_bytes': (60, 2, 2, 40, 3, 2, 1, 'safe', True, True),
    'safe_cost_bytes_floating': (60, 2, 2, 40, 3, 2, 3, 'safe', True, True),
    'no_model_noise': (60, 2, 2, 40, 3, 2, 1, 'cem', False, True),                 # sampling_propagation False: model noise exactly 0, actions still drawn
    'obs_not_quad_aligned': (58, 2, 2, 40, 3, 2, 1, 'cem', True, False),           # a quad with observation AND action features: generic on both
}


@pytest.mark.parametrize('case', sorted(CASES))
def test_lean_rollout_is_bit_identical_to_the_generic_kernels(case, monkeypatch):
    _torch()
    O, A, E, N, H, I, segs, variant, sampling, lean = CASES[case]
    pb = hp.make_problem(O, A, E, 4, seed=77)
    ref, new = _compare(monkeypatch, pb, I, lean=lean, N=N, H=H, P=E, E=E, k=max(2, N // 10), I=I, variant=variant, post=0.3,
                        sampling=sampling, chunks_per_tile=1, rollout_segments=segs)
    n_seg = new['segments'][0]
    assert (n_seg > 1) == (segs > 1)
    if case == 'pinned_and_floating':
        assert new['tiles'] == 264
    if variant == 'safe':
        assert ref['its'][0]['costs'].size == H * E * N


def test_lean_rollout_at_the_headline_shape(monkeypatch):
    """B2 itself (obs 60, act 2, K = P = E = 5, N = 2000, H = 30, I = 5, the automatic tile and segment plan): two iterations compared
    kernel by kernel, the whole plan through the graph; still two launches per iteration."""
    _torch()
    pb = hp.make_problem(60, 2, 5, 4, seed=77)
    ref, new = _compare(monkeypatch, pb, 2, N=2000, H=30, P=5, E=5, k=200, I=5)
    assert new['launches'] == 2 and new['graph_status'] == 'graph'
    assert new['segments'][0] > 1
