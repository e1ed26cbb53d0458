"""The lean one-chunk rollout (csrc/cem_rollout_lean.hip) on the cases of tests/lean_cases.py — the horizons at which its
two-steps-per-round loop leaves early or resumes at an odd step, both sides of its LDS allowance, action quads spread over two waves
and up to the eight there can be, action boxes whose bounds differ in every quad, every scorer branch through the hand-over:

 (a) every case BIT FOR BIT against the generic kernels (tests/test_gpu_lean_rollout.py's _compare: the reference handle is created
     under CEM_FORCE_ROLLOUT=generic; every iteration kernel by kernel, then the whole plan through the graph; rollout_path() asserted
     on both handles); the box cases' iteration-0 actions also against the oracle's sample of the plan's dumped action noise;
 (b) the scorer cases' iteration 0 on Philox against the fp64 oracle (oracle/cem_oracle.py — not project kernel code) on the streams
     that plan consumed, at the parity suite's own tolerance;
 (c) the largest-LDS handle replaying a second plan through its captured graph.

tests/test_lean_cases_cpu.py shows on the host that the table is what it claims and that the fp64 reference alone meets (b)'s
conditions with a margin."""
import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import helpers as hp
from tests import lean_cases as lc
from tests.test_gpu_lean_rollout import _compare
from tests.test_gpu_parity import ATOL

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _planner(monkeypatch, case, force=None, **extra):
    """The case's planner, created under CEM_FORCE_ROLLOUT=`force` or left automatic; the path it reports is the one expected."""
    if force:
        monkeypatch.setenv('CEM_FORCE_ROLLOUT', force)
    else:
        monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    pb = lc.problem(case)
    ocfg, pcfg = hp.configs(pb, **dict(lc.config_kwargs(case), **extra))
    pl = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    assert pl.rollout_path() == ('generic' if force == 'generic' else case.path)
    return pb, ocfg, pl


# ------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize('case', lc.CASES, ids=lambda c: c.name)
def test_lean_edge_case_is_bit_identical_to_the_generic_kernels(case, monkeypatch):
    _torch()
    pb = lc.problem(case)
    ref, new = _compare(monkeypatch, pb, case.I, lean=case.path == 'lean', **lc.config_kwargs(case))
    assert new['segments'] == case.plan
    if case.name == 'h7_pinned_and_floating':
        assert new['tiles'] == 264
    if case.variant == 'safe':
        assert ref['its'][0]['costs'].size == case.H * case.E * case.N
    if not case.box:
        return
    # The clip's operands per dimension: the lean handle's iteration-0 actions are the oracle's sample of the action noise that plan
    # consumed, bit for bit, and the clip is live on both sides of every dimension (white noise at sigma0 = (high - low) / 2 clips
    # about 16 % of the draws on either side)
    _, _, pl = _planner(monkeypatch, case)
    ea0 = pl.fill_noise(lc.PLAN_SEED, lc.PLAN_CALL)[0][0].cpu().numpy()
    pl.close()
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    shape = (case.H, case.act)
    a0 = new['its'][0]['actions'].reshape(case.N, case.H, case.act)
    np.testing.assert_array_equal(a0, o.sample_actions(np.broadcast_to(mu0, shape), np.broadcast_to(sg0, shape), lb, ub, ea0))
    assert np.all(a0 >= lb) and np.all(a0 <= ub)
    for a in range(case.act):
        if sg0[a] > 0:
            assert (a0[..., a] == lb[a]).any() and (a0[..., a] == ub[a]).any(), (case.name, a)
            assert ((a0[..., a] > lb[a]) & (a0[..., a] < ub[a])).mean() > 0.3, (case.name, a)
        else:
            assert np.all(a0[..., a] == lb[a])


# ------------------------------------------------------------------------------------------------- (b)
_ORACLE = {}        # scorer name -> the dumped streams and their fp64 rollout (the same for both objectives and segmentations)


def _oracle(case, ea0, em0):
    if case.scorer not in _ORACLE:
        _ORACLE[case.scorer] = (ea0, em0) + lc.oracle_iteration0(case, ea0, em0)
    ea_c, em_c, actions, ref64, traj64 = _ORACLE[case.scorer]
    np.testing.assert_array_equal(ea0, ea_c)            # (seed, call) name the streams: the objective and the segment plan do not
    np.testing.assert_array_equal(em0, em_c)
    return actions, traj64


@pytest.mark.parametrize('case', lc.SCORER_CASES, ids=lambda c: c.name)
def test_lean_scores_match_the_fp64_oracle(case, monkeypatch):
    """Iteration 0 of the lean handle's Philox plan against o.candidate_scores in fp64 on the streams cem_fill_noise dumps for that
    (seed, call): per-candidate scores within test_gpu_parity's ATOL (near-threshold candidates by hp.assert_scores_match_oracle's
    admissible outcomes), at least 80 % of the candidates clear of every threshold (test_rollout_scorer_branches' cap), SafeCemMpc's
    done-masked per-step cost bytes of the clear rows exactly, and the branch the case is about live.  With three segments the done /
    d_prev / c_prev / cum quad goes through two hand-overs."""
    torch = _torch()
    pb, ocfg, pl = _planner(monkeypatch, case)
    assert pl.rollout_path() == 'lean' and pl.segments() == case.plan
    P, N, H = case.E, case.N, case.H
    ea, em, _ = pl.fill_noise(lc.PLAN_SEED, lc.PLAN_CALL)
    ea0, em0 = ea[0].cpu().numpy(), em[0].cpu().numpy()
    pl.plan_begin(pb['state'], seed=lc.PLAN_SEED, call=lc.PLAN_CALL)
    pl.plan_rollout(0)
    torch.cuda.synchronize()
    actions = pl.actions().cpu().numpy().reshape(N, H, case.act).copy()
    scores = pl.scores_local().cpu().numpy().copy()
    gpu_costs = pl.costs().cpu().numpy().reshape(H, P * N).astype(np.float64) if case.variant == 'safe' else None
    pl.plan_select(0)
    pl.plan_end()
    pl.close()
    ref_actions, traj64 = _oracle(case, ea0, em0)
    np.testing.assert_array_equal(actions, ref_actions)
    sp = pb['scorer']
    row_ok = o.threshold_margins(traj64, sp) > 1e-4
    ok = row_ok.reshape(P, N).all(axis=0)
    print('%s: %d of %d candidates clear of every threshold' % (case.name, ok.sum(), N))
    assert ok.mean() > 0.8, 'too many candidates on a threshold for a meaningful test'
    err, n_near, n_flip = hp.assert_scores_match_oracle(scores, traj64, P, N, sp, case.variant, ocfg.posterior_mean_threashold, ATOL, case.name)
    print('%s: max|gpu-f64| = %.3g; %d of %d candidates near a threshold (%d flipped)' % (case.name, err, n_near, N, n_flip))
    ref_costs, first_goal = lc.masked_costs_and_first_goal(traj64, sp)
    if case.variant == 'safe':
        np.testing.assert_array_equal(gpu_costs[:, row_ok], ref_costs[:, row_ok])
    if sp.cost_kinds:
        assert ref_costs.max() >= 1 and (ref_costs == 0).any()
        if not sp.constrain_indicator and len(sp.cost_kinds) > 1:
            assert ref_costs.max() >= 2, 'the non-indicator sum should exceed 1 somewhere'
    if case.scorer == 'active_reward_clip':
        r, _ = o.reward(traj64[:, 0], traj64[:, 1], sp)
        assert (np.abs(r) == sp.reward_clip).mean() > 0.3
    if not sp.observe_goal_lidar:
        assert (first_goal < H).any(), 'goal_dist case should reach the goal'
        assert (first_goal < 3).any() and ((first_goal >= 3) & (first_goal < 6)).any() and (first_goal == 6).any()      # in every segment


# ------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize('name', ['lds_1quad_h52', 'lds_1quad_h52_four_segments'])
def test_the_largest_lds_launch_replays_through_its_graph(name, monkeypatch):
    """H = 52 with one action quad: the kernel's largest dynamic LDS and longest parking area.  Launch count and graph status are the
    generic reference's, and a plan with another seed and call replayed through the captured graph is bit-identical to it again."""
    torch = _torch()
    case = lc.BY_NAME[name]
    assert lc.act_lds_bytes(case.H, case.act) == 16112
    pb, _, ref = _planner(monkeypatch, case, 'generic', use_graph=True)
    _, _, new = _planner(monkeypatch, case, None, use_graph=True)
    assert new.rollout_path() == 'lean' and ref.rollout_path() == 'generic'
    assert new.launches_per_iteration() == ref.launches_per_iteration() and new.segments() == ref.segments() == case.plan
    results = []
    for seed, call in ((lc.PLAN_SEED, lc.PLAN_CALL), (lc.PLAN_SEED, lc.PLAN_CALL), (11, 8)):       # capture, replay, replay with other streams
        ar, sr, ir = ref.plan(pb['state'], seed=seed, call=call)
        an, sn, inn = new.plan(pb['state'], seed=seed, call=call)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(an, ar)
        assert sn == sr and inn == ir == case.I and np.isfinite(sn)
        for view in ('actions', 'returns', 'scores_local', 'mu_sigma', 'elite_idx') + (('costs',) if case.variant == 'safe' else ()):
            assert torch.equal(getattr(new, view)(), getattr(ref, view)()), (view, seed, call)
        results.append((an.copy(), new.actions().cpu().numpy().copy()))
    assert new.graph_status() == ref.graph_status() == 'graph'
    np.testing.assert_array_equal(results[0][1], results[1][1])                  # the replay reproduces the captured plan
    assert not np.array_equal(results[2][1], results[1][1])                      # and another (seed, call) is another plan
    ref.close(); new.close()
