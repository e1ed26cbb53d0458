"""The two forms of the lean one-chunk rollout — the branchy one (csrc/cem_rollout_lean.hip) and the straight-line one
(csrc/cem_rollout_lean_straight.hip: the objective a template parameter, the weight ring's positions constants, no rare scorer kinds)
— against each other and against the generic kernels, on every case of tests/lean_cases.py that runs lean, plus sampling_propagation
False on both objectives.  Each case runs three ways: the automatic choice, CEM_FORCE_ROLLOUT=lean_branchy and =generic at create.
Between all three, BIT FOR BIT (assert_array_equal, no tolerance: the same operations on the same data): per-row returns, cost bytes,
stored actions, scores, mu / sigma and the elite set after every iteration kernel by kernel, then the whole plan through its graph.

Which form the automatic handle reports (CemPlanner.rollout_form, cem_planner_rollout_form) is asserted for every iteration: 2, the
straight-line form, where the scorer has its goal as a lidar kind and at most one constrained cost kind; 1 otherwise.  Of
hp.SCORER_CASES that puts
    straight-line:  one_kind_sum, no_cost_kinds, no_reward_clip, active_reward_clip
    branchy:        two_kinds, three_kinds, four_kinds, four_kinds_sum (more than one kind), goal_dist (observe_goal_dist),
                    goal_dist_sum3 (both)
and every case without a scorer of its own (one hazards kind, goal lidar) on the straight-line side.  The table already resumes a
segment at an odd step on both objectives (h5_resumed_at_an_odd_step[_safe], lds_1quad_h52_four_segments)."""
import numpy as np
import pytest

from tests import helpers as hp
from tests import lean_cases as lc

pytestmark = pytest.mark.gpu

STRAIGHT_SCORERS = {'one_kind_sum', 'no_cost_kinds', 'no_reward_clip', 'active_reward_clip'}
BRANCHY_SCORERS = {'two_kinds', 'three_kinds', 'four_kinds', 'four_kinds_sum', 'goal_dist', 'goal_dist_sum3'}

# sampling_propagation False (model noise exactly 0, the actions still drawn), unsegmented and resumed at an odd step, both objectives
NO_NOISE = [lc.Case('no_model_noise_%s_%dseg' % (variant, segments), 'sampling', 60, 2, 2, 40, 5, 2, segments, variant, None, None, 4, 'lean',
                    (segments, -(-5 // segments)))
            for variant in ('cem', 'safe') for segments in (1, 2)]
LEAN_CASES = [c for c in lc.CASES if c.path == 'lean']
VIEWS = ('returns', 'costs', 'actions', 'scores', 'mu_sigma', 'elites')


def want_form(case):
    if case.scorer is None:
        return 2
    spec = hp.SCORER_CASES[case.scorer]
    return 2 if spec.get('observe_goal_lidar', True) and len(spec['kinds']) <= 1 else 1


def _snapshot(pl, safe):
    out = dict(returns=pl.returns().cpu().numpy().copy(), actions=pl.actions().cpu().numpy().copy(), mu_sigma=pl.mu_sigma().cpu().numpy().copy(),
               scores=pl.scores_local().cpu().numpy().copy(), elites=pl.elite_idx().cpu().numpy().copy(),
               costs=pl.costs().cpu().numpy().copy() if safe else np.zeros(0, np.uint8))
    return out


def _run(monkeypatch, case, force, **extra):
    """One planner of the case, created under CEM_FORCE_ROLLOUT=`force` (None: automatic): every iteration kernel by kernel with all it
    leaves behind, then the same plan as one call through the captured graph."""
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    if force:
        monkeypatch.setenv('CEM_FORCE_ROLLOUT', force)
    else:
        monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    pb = lc.problem(case)
    _, pcfg = hp.configs(pb, use_graph=True, **dict(lc.config_kwargs(case), **extra))
    pl = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    safe = case.variant == 'safe'
    out = dict(path=pl.rollout_path(), forms=[pl.rollout_form(it) for it in range(case.I)], segments=pl.segments(),
               launches=pl.launches_per_iteration(), its=[])
    pl.plan_begin(pb['state'], seed=lc.PLAN_SEED, call=lc.PLAN_CALL)
    for it in range(case.I):
        pl.plan_rollout(it)
        pl.plan_select(it)
        out['its'].append(_snapshot(pl, safe))
    out['end'] = pl.plan_end()
    out['plan'] = pl.plan(pb['state'], seed=lc.PLAN_SEED, call=lc.PLAN_CALL)
    out['graph_status'] = pl.graph_status()
    out['after_plan'] = _snapshot(pl, safe)
    pl.close()
    return out


def _assert_same(a, b, what):
    assert (a['segments'], a['launches'], a['graph_status']) == (b['segments'], b['launches'], b['graph_status']), what
    for it, (x, y) in enumerate(zip(a['its'], b['its'])):
        for key in VIEWS:
            np.testing.assert_array_equal(x[key], y[key], err_msg='%s: %s after iteration %d' % (what, key, it))
    for key in ('end', 'plan'):
        np.testing.assert_array_equal(a[key][0], b[key][0], err_msg='%s: %s' % (what, key))
        assert a[key][1] == b[key][1] and a[key][2] == b[key][2], (what, key)
    for key in VIEWS:
        np.testing.assert_array_equal(a['after_plan'][key], b['after_plan'][key], err_msg='%s: %s after the whole plan' % (what, key))


def _three_ways(monkeypatch, case, **extra):
    generic = _run(monkeypatch, case, 'generic', **extra)
    branchy = _run(monkeypatch, case, 'lean_branchy', **extra)
    auto = _run(monkeypatch, case, None, **extra)
    assert generic['path'] == 'generic' and generic['forms'] == [0] * case.I
    assert branchy['path'] == 'lean' and branchy['forms'] == [1] * case.I
    assert auto['path'] == 'lean' and auto['forms'] == [want_form(case)] * case.I, (case.name, auto['forms'])
    assert auto['segments'] == case.plan
    assert np.isfinite(generic['its'][0]['returns']).all() and np.isfinite(generic['its'][0]['scores']).all()
    _assert_same(generic, branchy, 'generic vs lean_branchy')
    _assert_same(branchy, auto, 'lean_branchy vs automatic')
    _assert_same(generic, auto, 'generic vs automatic')
    return auto


def test_the_scorer_cases_fall_on_both_sides():
    assert STRAIGHT_SCORERS | BRANCHY_SCORERS == set(hp.SCORER_CASES) and not STRAIGHT_SCORERS & BRANCHY_SCORERS
    for c in lc.SCORER_CASES:
        assert want_form(c) == (2 if c.scorer in STRAIGHT_SCORERS else 1), c.name
    assert {want_form(c) for c in LEAN_CASES} == {1, 2}


@pytest.mark.parametrize('case', LEAN_CASES, ids=lambda c: c.name)
def test_lean_forms_and_generic_kernels_agree_bit_for_bit(case, monkeypatch):
    auto = _three_ways(monkeypatch, case)
    if case.variant == 'safe':
        assert auto['its'][0]['costs'].size == case.H * case.E * case.N


@pytest.mark.parametrize('case', NO_NOISE, ids=lambda c: c.name)
def test_lean_forms_agree_without_model_noise(case, monkeypatch):
    auto = _three_ways(monkeypatch, case, sampling=False)
    assert auto['forms'] == [2] * case.I
