"""CemMpc / SafeCemMpc with replan_every and plan_readout, on a stand-in planner (no GPU): which decisions plan, which follow the kept
sequence, what reset() does, how the Philox call numbers advance, and the refusals."""
import numpy as np
import pytest

from ethz_safe_learning_amd.planner import PlanReadout
from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
from ethz_safe_learning_amd.simba.spaces import Box

F = np.float32
H, A, P = 5, 2, 3


class _Env:
    action_space = Box(-np.ones(A, F), np.ones(A, F))


class _Planner:
    """What the policies ask of a handle: plan numbers its plans, the read-out's sequence of plan p is 100 p + step."""
    h = object()
    max_batch = 1

    def __init__(self, score=1.0):
        self.plans, self.noise_calls, self._call, self.score = [], [], 0, score

    def take_calls(self, n=1):
        first = self._call
        self._call += int(n)
        return np.arange(first, first + int(n), dtype=np.uint64)

    def plan(self, state, seed=0, call=None):
        if call is None:
            call = int(self.take_calls()[0])
        self.plans.append(int(call))
        return self._sequence()[0].copy(), self.score, 3

    def _sequence(self):
        p = len(self.plans)
        return (100.0 * p + np.arange(H, dtype=F)[:, None] + np.array([0.0, 0.5], F)[None]).astype(F)

    def plan_readout(self, problem=0):
        return PlanReadout(self._sequence(), F(self.score), 4, 1, np.zeros(P, F), np.zeros(H, np.int32), 0)

    def output_noise(self, seed=0, call=0):
        self.noise_calls.append(int(call))
        return np.array([1.0, -1.0], F)


def _policy(cls=CemMpc, planner=None, **kw):
    base = dict(model=None, environment=_Env(), horizon=H, iterations=3, smoothing=0.0, n_samples=64, n_elite=8, particles=P,
                stddev_threshold=-1.0, noise_stddev=0.0)
    if cls is SafeCemMpc:
        base['posterior_mean_threashold'] = 0.15
    base.update(kw)
    pol = cls(**base)
    pol._planner = planner if planner is not None else _Planner()
    pol.build = lambda: None                                  # (the handle is the stand-in; nothing to create or stage)
    return pol


def test_replan_every_three_plans_at_decisions_0_3_6_and_follows_the_sequence_in_between():
    pol = _policy(replan_every=3)
    assert pol.plan_readout                                    # implied
    acts = [pol.generate_action(np.zeros(4, F)) for _ in range(7)]
    pl = pol._planner
    assert pl.plans == [0, 3, 6]                               # plans at decisions 0, 3, 6 — with the call numbers of those decisions
    assert pl._call == 7                                       # every decision consumed one call number
    for d, a in enumerate(acts):
        p, j = d // 3 + 1, d % 3
        np.testing.assert_array_equal(a, np.array([100.0 * p + j, 100.0 * p + j + 0.5], F))
        assert a.dtype == F
    assert pl.noise_calls == []                                # noise_stddev = 0: no draw, exact copies
    assert pol.last_plan.candidate == 4 and pol.last_score == 1.0 and pol.last_iterations == 3
    # a returned action is a copy: writing to it does not reach the kept sequence
    pol2 = _policy(replan_every=2)
    pol2.generate_action(np.zeros(4, F))
    a = pol2.generate_action(np.zeros(4, F))
    a[:] = -7
    assert pol2.last_plan.sequence[1, 0] == 101.0


def test_reset_discards_the_kept_sequence():
    pol = _policy(replan_every=3)
    pol.generate_action(np.zeros(4, F))
    pol.generate_action(np.zeros(4, F))
    pol.reset()
    a = pol.generate_action(np.zeros(4, F))
    assert pol._planner.plans == [0, 2]
    np.testing.assert_array_equal(a, np.array([200.0, 200.5], F))
    b = pol.generate_action(np.zeros(4, F))
    np.testing.assert_array_equal(b, np.array([201.0, 201.5], F))


def test_the_output_noise_of_a_followed_decision_is_that_decisions_own_call():
    pol = _policy(replan_every=2, noise_stddev=0.25)
    pol.generate_action(np.zeros(4, F))
    a = pol.generate_action(np.zeros(4, F))
    pol.generate_action(np.zeros(4, F))
    assert pol._planner.plans == [0, 2] and pol._planner.noise_calls == [1]
    np.testing.assert_array_equal(a, np.array([101.0, 101.5], F) + np.array([1.0, -1.0], F) * F(0.25))


def test_warm_started_decisions_number_their_calls_per_environment():
    pol = _policy(replan_every=2, warm_start=True, warm_shift=2, noise_stddev=0.5)
    pol.reset = lambda: None
    pol.slot = 3
    for _ in range(4):
        pol.generate_action(np.zeros(4, F))
    assert pol._planner.plans == [(3 << 32) + 0, (3 << 32) + 2] and pol._planner.noise_calls == [(3 << 32) + 1, (3 << 32) + 3]


def test_replan_every_one_and_plan_readout_alone_plan_at_every_decision():
    pol = _policy(plan_readout=True)
    for _ in range(3):
        pol.generate_action(np.zeros(4, F))
    assert pol._planner.plans == [0, 1, 2] and pol.last_plan.sequence[0, 0] == 300.0
    seq = pol.generate_action_sequence(np.zeros(4, F))
    assert seq.shape == (H, A) and seq[0, 0] == 400.0 and pol._planner.plans == [0, 1, 2, 3]
    off = _policy()
    off.generate_action(np.zeros(4, F))
    assert off.last_plan is None and not off.plan_readout and off._readout_config() == {} and pol._readout_config() == dict(plan_readout=True)
    with pytest.raises(ValueError, match='plan_readout'):
        off.generate_action_sequence(np.zeros(4, F))


def test_generate_action_sequence_plans_even_while_a_sequence_is_being_followed():
    pol = _policy(replan_every=3)
    pol.generate_action(np.zeros(4, F))
    seq = pol.generate_action_sequence(np.zeros(4, F))
    assert pol._planner.plans == [0, 1] and seq[0, 0] == 200.0
    np.testing.assert_array_equal(pol.generate_action(np.zeros(4, F)), seq[1])     # ... and that plan is the one in force


def test_the_three_refusals():
    with pytest.raises(ValueError, match='replan_every'):
        _policy(replan_every=0)
    with pytest.raises(ValueError, match='replan_every'):
        _policy(replan_every=H + 1)
    with pytest.raises(ValueError, match='replan_every'):
        _policy(replan_every=1.5)
    assert _policy(replan_every=H).replan_every == H
    with pytest.raises(ValueError, match='warm_shift'):
        _policy(replan_every=2, warm_start=True, warm_shift=1)
    with pytest.raises(ValueError, match='warm_shift'):
        _policy(replan_every=3, keep_elites=0.3, shift_elites=True, warm_shift=2)
    assert _policy(replan_every=2, warm_start=True, warm_shift=2).replan_every == 2
    assert _policy(replan_every=2, keep_elites=0.3).replan_every == 2              # elites kept inside a plan only: nothing is shifted
    pol = _policy(replan_every=2)
    with pytest.raises(ValueError, match='replan_every'):
        pol.generate_actions(np.zeros((2, 4), F))


def test_safe_policy_keeps_the_sequence_of_the_plan_whose_action_it_returns():
    reward, cost = _Planner(score=-80.0), _Planner(score=-0.2)
    cost.plans = [None] * 6                                    # (its sequences start at 700: told apart from the reward handle's)
    pol = _policy(SafeCemMpc, planner=reward, replan_every=2, recover_below=-50.0)
    pol._cost_planner = cost
    pol.build_cost = lambda: cost
    a0 = pol.generate_action(np.zeros(4, F))
    assert pol.last_recovered and a0[0] == 700.0               # the recovery plan's action
    assert pol.last_plan.sequence[0, 0] == 700.0               # ... and its read-out
    a1 = pol.generate_action(np.zeros(4, F))
    np.testing.assert_array_equal(a1, np.array([701.0, 701.5], F))
    assert reward.plans == [0] and cost.plans[6:] == [0]       # the cost plan took the replaced plan's call number
    reward.score = 5.0                                         # no recovery this time: the reward plan's sequence is kept
    a2 = pol.generate_action(np.zeros(4, F))
    a3 = pol.generate_action(np.zeros(4, F))
    assert not pol.last_recovered and reward.plans == [0, 2] and a2[0] == 200.0 and a3[0] == 201.0
    plain = _policy(SafeCemMpc, replan_every=2)
    acts = [plain.generate_action(np.zeros(4, F)) for _ in range(4)]
    assert plain._planner.plans == [0, 2] and [float(a[0]) for a in acts] == [100.0, 101.0, 200.0, 201.0]
