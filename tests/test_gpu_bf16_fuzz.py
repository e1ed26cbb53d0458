"""Randomised shapes for the precision='bf16' rollout on the GPU: the corners of tests/test_gpu_fuzz.py that the kernel takes — every
depth and tile size, padded widths, obs + act on either side of the layer-0 chunk counts, one-row tail tiles, members that split a
particle, sampling / scaling off, unbounded boxes, both objectives — held to the kernel's OWN arithmetic at the bars of
tests/bf16_cases.py.  The seeds are the committed tables of tests/bf16_fuzz_cases.py, screened on the CPU by
tests/test_bf16_fuzz_cpu.py: a seed that fails here is a finding about the kernel (the case dict is printed)."""
import numpy as np
import pytest

from tests import bf16_cases as bc
from tests import bf16_fuzz_cases as fz
from tests import helpers as hp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _shown(c):
    return {k: v for k, v in c.items() if k not in ('low', 'high')}


@pytest.mark.parametrize('seed', fz.SCORE_SEEDS)
def test_random_shape_scores_follow_the_rounding_model(torch, seed):
    """One iteration in planning mode on explicit noise: sampled actions bit for bit, scores under bf16_cases.check_scores against
    candidate_scores under the emulation."""
    ref = fz.score_case(seed)
    c, pb = ref['c'], ref['pb']
    pl = hp.make_planner(pb, ref['pcfg'])
    pl.plan_begin(pb['state'], eps_act=ref['ea'], eps_model=ref['em'])
    pl.plan_rollout(0)
    torch.cuda.synchronize()
    sc = pl.scores_local().cpu().numpy().copy()
    actions = pl.actions().cpu().numpy().copy()
    pl.plan_end()
    rc = pl.tiles()[0]
    pl.close()
    what = 'bf16 score seed %d %s' % (seed, _shown(c))
    assert c['rc'] in (0, rc), what
    np.testing.assert_array_equal(actions, ref['actions'], err_msg=what)
    print('%s rc %d: %s' % (what, rc, bc.score_figures(sc, ref)))
    ratio, near, med, p90 = bc.check_scores(sc, ref, what)
    print('bf16 score seed %d: score ratio %.4f, %.1f %% near a threshold; flip-free median ratio %.4f, 90th percentile ratio %.4f' % (seed, ratio, 100 * near, med, p90))


@pytest.mark.parametrize('seed', fz.UNFOLD_SEEDS)
def test_random_shape_unfold_and_moments_follow_the_rounding_model(torch, seed):
    """unfold_sequences(..., return_moments=True) on per-row start states: traj[:, 0] is s0, and the trajectory, mu and sd — as [B, H, O]
    tensors, per step — meet the rounding model against bf16_cases.unfold_with_moments under the emulation and the fp64 oracle."""
    u = fz.unfold_case(seed)
    pl = hp.make_planner(u['pb'], u['pcfg'])
    got = tuple(x.cpu().numpy() for x in pl.unfold_sequences(u['s0'], u['acts'], eps_model=u['eps'], return_moments=True))
    pl.close()
    what = 'bf16 unfold seed %d %s' % (seed, u['c'])
    for name, g, e, r in zip(('trajectory', 'mu', 'sd'), got, u['emu'], u['ref64']):
        first = 1 if name == 'trajectory' else 0
        print('%s %s: RMS(kernel - emulation) per step %s | RMS(emulation - fp64) %s' % (
            what, name, ' '.join('%.2e' % bc.rms(g[:, t] - e[:, t]) for t in range(first, g.shape[1])),
            ' '.join('%.2e' % bc.rms(e[:, t] - r[:, t]) for t in range(first, g.shape[1]))))
    worst = fz.check_unfold(got, u, what)
    print('bf16 unfold seed %d: largest ratios trajectory %.4f mu %.4f sd %.4f' % (seed, *worst))


@pytest.mark.parametrize('seed', fz.CUT_SEEDS)
def test_random_shape_shard_and_tile_invariance(torch, seed):
    """Philox mode: scores, per-row returns and cost bytes of W in {2, 3, 4} rank shards at one tile size concatenate to the single
    rank's at another, bit for bit (tests/test_gpu_fuzz.py's invariance, in the bf16 kernel's own tile set-up and bookkeeping)."""
    c, pb, cfgs = fz.cut_configs(seed)
    W, P, N, H = c['W'], c['P'], c['N'], c['H']

    def run(key):
        pl = hp.make_planner(pb, cfgs[key])
        pl.plan_begin(pb['state'], seed=77, call=seed)
        pl.plan_rollout(0)
        torch.cuda.synchronize()
        out = (pl.scores_local().cpu().numpy().copy(), pl.returns().cpu().numpy().copy(),
               pl.costs().cpu().numpy().copy() if c['variant'] == 'safe' else None)
        pl.plan_end()
        pl.close()
        return out
    what = 'bf16 cut seed %d %s' % (seed, _shown(c))
    full = run((1, 0))
    assert np.isfinite(full[0]).all(), what
    parts = [run((W, r)) for r in range(W)]
    np.testing.assert_array_equal(np.concatenate([p_[0] for p_ in parts]), full[0], err_msg=what)
    Nl = N // W                                               # per-row returns are particle-major within a rank: [P][N / W]
    np.testing.assert_array_equal(np.concatenate([p_[1].reshape(P, Nl) for p_ in parts], axis=1).reshape(-1), full[1].reshape(-1), err_msg=what)
    if c['variant'] == 'safe':
        cost = np.concatenate([p_[2].reshape(H, P, Nl) for p_ in parts], axis=2).reshape(H, -1)
        np.testing.assert_array_equal(cost, full[2].reshape(H, -1), err_msg=what)
