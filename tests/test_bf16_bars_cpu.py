"""Do the bars of the precision='bf16' GPU tests have teeth?  Emulations that are wrong in ONE way each (bf16_cases.mutant) are put in
the kernel's place on every fixed case tests/test_gpu_bf16.py relies on — the trajectory cases of test 2, the score cases of test 3, the
scorer-branch cases — and must FAIL, while the fp32-accumulating stand-ins pass (the random-shape cases: tests/test_bf16_fuzz_cpu.py).

Which bar catches which mutant (counted by these tests: cases of test 3 out of 4 / scorer-branch cases out of 40):
  scores (bf16_cases.check_scores)        RMS      max      median   90th percentile   near-threshold outcomes
    trunc_act                             4 / 39   3 / 39   4 / 40   4 / 40            0 / 12
    trunc_w                               4 / 40   3 / 36   4 / 40   4 / 40            0 / 12
    raw_input                             1 / 39   0 / 0    4 / 40   4 / 40            0 / 0
    raw_heads                             2 / 34   1 / 0    4 / 40   4 / 40            0 / 0
    drop_chunk                            4 / 40   4 / 40   4 / 40   4 / 40            2 / 22
    bias_bf16                             4 / 39   0 / 36   4 / 40   4 / 40            0 / 12
    raw_var                               none: scores see the variance head only through sigma eps; its ratios are the stand-ins'
  So the two quantile bars over the flip-free candidates catch every mutant the scores can see on EVERY case; the RMS bar over the
  clear candidates misses the unrounded layer-0 input on 3 of test 3's 4 cases and the unrounded heads' input on 2 (at obs 100 they
  shift the scores by 0.15 - 0.3 of the rounding's own size, far below a yardstick that one flipped goal reward or safe penalty
  inflates 20 to 10 000 times), and the max bar never sees them.
  trajectories (bf16_cases.check_rounding_model on test 2's 3 cases)
    every mutant but raw_var: the RMS bar at step 1 already; raw_var: passes (largest ratio 0.003 - 0.04: the states see sigma eps only)
  moments
    raw_var: the sd comparison of the exact cases (below), and sd under the rounding model on every random-shape unfold case
    (tests/test_bf16_fuzz_cpu.py)
With check_scores reverted to its RMS and max conditions over the clear candidates alone, test_score_bars_fail_every_mutant fails
(obs100-cem: the raw_input mutant passes every bar of the score check)."""
import functools

import numpy as np
import pytest

from tests import bf16_cases as bc
from tests import helpers as hp

SCORE_MUTANTS = [k for k in bc.MUTANTS if k not in bc.SCORE_BLIND]


def _assert_yardstick(c, what):
    """the flip-free yardstick is the bf16 rounding's own size: neither vacuous nor inflated"""
    Y = bc.flip_free_set(c)
    m = bc.rms((c['emu'].astype(np.float64) - c['ref64'])[Y])
    assert 1e-5 < m < 2e-3, '%s: RMS(emulation - fp64) over the flip-free candidates %.3e' % (what, m)
    return m, float(Y.mean())


def _mutants_fail(c, what):
    caught = {k: bc.failed_score_bars(bc.scores_under(c, bc.mutant(k)), c) for k in bc.MUTANTS}
    print('%s: %s' % (what, ', '.join('%s: %s' % (k, '+'.join(v) or 'passes') for k, v in caught.items())))
    for k in SCORE_MUTANTS:
        assert caught[k], '%s: the %s mutant passes every bar of the score check' % (what, k)
    for k in SCORE_MUTANTS:
        assert {'median', 'p90'} & set(caught[k]), '%s: the %s mutant passes both quantile bars' % (what, k)
    return caught


@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('O,A', [(60, 2), (100, 12)], ids=['obs60', 'obs100'])
def test_score_bars_fail_every_mutant(O, A, variant):
    """GPU test 3's cases: every mutant the scores can see misses a bar (a quantile bar at the least), and the yardstick of the
    quantile bars lies in (1e-5, 2e-3) with at least Y_MIN of the candidates behind it.  (The stand-ins: tests/test_bf16_cpu.py.)"""
    c = bc.score_case(O, A, variant)
    what = 'obs %d %s' % (O, variant)
    m, y = _assert_yardstick(c, what)
    print('%s: flip-free %.1f %%, RMS(emulation - fp64) over them %.3e (over all clear candidates %.3e)' % (
        what, 100 * y, m, bc.rms((c['emu'].astype(np.float64) - c['ref64'])[~c['near']])))
    _mutants_fail(c, what)


@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_trajectory_bars_fail_every_mutant(dims):
    """GPU test 2's cases: every mutant that moves mu misses the RMS or the max condition at some step."""
    _, _, _, _, emu, ref64 = bc.traj_case(dims)
    for k in bc.MUTANTS:
        traj = bc.traj_under(dims, bc.mutant(k))
        try:
            failed = ''
            print('obs %d: %s passes, largest ratio %.4f' % (dims[0], k, max(bc.check_rounding_model(traj, emu, ref64, 'obs %d %s' % (dims[0], k)))))
        except AssertionError as e:
            failed = str(e)
            print('obs %d: %s fails: %s' % (dims[0], k, failed[:160]))
        assert failed or k in bc.SCORE_BLIND, 'obs %d: the %s mutant passes the trajectory bars' % (dims[0], k)


@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_exact_cases_catch_the_variance_head_mutant(dims):
    """GPU test 1's sd comparison (rtol = atol = 2e-5) on bf16_cases.exact_problem: the one mutant neither scores nor trajectories see —
    the variance head's input left unrounded — misses it, and the emulation in three summation orders meets it."""
    O, A, U = dims
    pb = bc.exact_problem(O, A, U, E=5, seed=O)
    s0, acts, eps = bc.exact_inputs(O, A, 40, 3, seed=O + 1)
    args = (s0, acts, pb['weights'], bc.members_of(40, 5), pb['inputs_min'], pb['inputs_max'], eps)
    with bc.emulating(bc.emu64):
        rs = bc.unfold_with_moments(*args)[2]
    for order in range(3):
        with bc.emulating(functools.partial(bc.emu32, order=order)):
            np.testing.assert_allclose(bc.unfold_with_moments(*args)[2], rs, rtol=2e-5, atol=2e-5)
    with bc.emulating(bc.mutant('raw_var')):
        sd = bc.unfold_with_moments(*args)[2]
    assert not np.allclose(sd, rs, rtol=2e-5, atol=2e-5), 'the raw_var mutant passes the sd comparison of the exact cases'


# ---- the scorer branches under bf16 (tests/test_gpu_bf16.py test_scorer_branches_follow_the_rounding_model) ------------------------------
@pytest.mark.parametrize('obs', [60, 84])
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('case', list(hp.SCORER_CASES))
def test_scorer_branch_bars_hold_the_stand_ins_and_fail_every_mutant(case, variant, obs):
    """Every helpers.SCORER_CASES entry at obs 60 (one input block per wave) and 84 (two), both objectives: at most NEAR_CAP of the
    candidates near a threshold, at least Y_MIN flip-free, the yardstick in range; every stand-in (24 chunk orders, four fine-grained
    sums) meets every bar; every mutant the scores can see misses one.  The branch must be live: costs of both values, a sum above 1 where kinds are summed, the goal reached
    under observe_goal_dist, the clip active where it is set."""
    c = bc.scorer_case(case, obs, variant)
    what = '%s obs %d %s' % (case, obs, variant)
    m, y = _assert_yardstick(c, what)
    worst = np.zeros(3)
    for name, forward in bc.stand_ins().items():              # all of them: bf16_cases.SCORER_NOISE_SEED says why
        ratio, near, med, p90 = bc.check_scores(bc.scores_under(c, forward), c, '%s %s' % (what, name))
        worst = np.maximum(worst, (ratio, med, p90))
    print('%s: %.1f %% near, %.1f %% flip-free, yardstick %.3e; largest stand-in ratios RMS %.4f median %.4f 90th percentile %.4f' % (what, 100 * near, 100 * y, m, *worst))
    _mutants_fail(c, what)
    sp, traj = c['pb']['scorer'], c['traj']
    from oracle import cem_oracle as o
    if variant == 'safe' and sp.cost_kinds:
        assert c['costs'].max() >= 1 and (c['costs'] == 0).any() and c['row_clear'].mean() > 0.8
        if not sp.constrain_indicator and len(sp.cost_kinds) > 1:
            assert c['costs'].max() >= 2, 'the non-indicator sum should exceed 1 somewhere'
    if case == 'active_reward_clip':
        assert (np.abs(o.reward(traj[:, 0], traj[:, 1], sp)[0]) == sp.reward_clip).mean() > 0.3
    if not sp.observe_goal_lidar:
        assert any(o.reward(traj[:, t], traj[:, t + 1], sp)[1].any() for t in range(traj.shape[1] - 1)), 'goal_dist case should reach the goal'
