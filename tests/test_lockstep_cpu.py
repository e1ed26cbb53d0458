"""BaseAgent.sample_trajectories_lockstep (no GPU): environments stepped side by side with one batched policy call per decision give,
environment by environment, exactly the records serial sample_trajectories gives — with one environment, with several that end at
different times, with action_repeat > 1, and with a policy that has only generate_action."""
import numpy as np
import pytest

from ethz_safe_learning_amd.simba.agents.agent import BaseAgent
from ethz_safe_learning_amd.simba.environment_utils.point_goal_env import PointGoalEnv


class LinearPolicy:
    """Deterministic: a fixed linear map of the observation, squashed into the action box."""

    def __init__(self, obs_dim, act_dim=2, seed=5):
        self.W = np.random.default_rng(seed).standard_normal((act_dim, obs_dim)).astype(np.float32) * 0.3
        self.calls, self.batch_sizes = 0, []

    def _act(self, state):
        return np.tanh(self.W @ np.asarray(state, np.float32)).astype(np.float32)

    def generate_action(self, state):
        self.calls += 1
        return self._act(state)


class BatchedLinearPolicy(LinearPolicy):
    def generate_actions(self, states):
        states = np.asarray(states, np.float32)
        self.batch_sizes.append(states.shape[0])
        return np.stack([self._act(st) for st in states])          # (row by row: the same rounding as generate_action)


def _agent(action_repeat):
    return BaseAgent(replay_buffer_size=1000, add_observation_noise=False, action_repeat=action_repeat)


def _env(seed, num_steps=1000, hazards=8):
    return PointGoalEnv(n_hazards=hazards, n_vases=1, num_steps=num_steps, seed=seed, config=dict(constrain_hazards=True))


def _assert_same_paths(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert set(g) == set(w)
        for key in ('observation', 'action', 'next_observation', 'terminal', 'reward'):
            np.testing.assert_array_equal(g[key], w[key], err_msg=key)
        assert g['info'] == w['info']


@pytest.mark.parametrize('action_repeat', [1, 3])
@pytest.mark.parametrize('policy_cls', [LinearPolicy, BatchedLinearPolicy])
def test_one_environment_matches_sample_trajectories(action_repeat, policy_cls):
    obs_dim = _env(0).reset().shape[0]
    serial_env, lock_env = _env(11, num_steps=40), _env(11, num_steps=40)
    agent = _agent(action_repeat)
    want, want_steps = agent.sample_trajectories(serial_env, policy_cls(obs_dim), batch_size=100, max_trajectory_length=25)
    got, got_steps = agent.sample_trajectories_lockstep([lock_env], policy_cls(obs_dim), batch_size=100, max_trajectory_length=25)
    assert len(want) > 1                                  # several episodes: the budget rule starts new ones
    assert got_steps == want_steps
    _assert_same_paths(got, want)


@pytest.mark.parametrize('action_repeat', [1, 2])
def test_k_environments_match_k_serial_runs(action_repeat):
    obs_dim = _env(0).reset().shape[0]
    lengths = [9, 30, 17, 30]                            # environments whose episodes end early (num_steps) and one cut at the max length
    seeds = [3, 4, 5, 6]
    agent = _agent(action_repeat)
    want, want_steps = [], 0
    for s, n in zip(seeds, lengths):                      # one episode each: the budget (1 step) starts no second episode
        paths, steps = agent.sample_trajectories(_env(s, num_steps=n), LinearPolicy(obs_dim), batch_size=1, max_trajectory_length=24)
        want += paths
        want_steps += steps
    pol = BatchedLinearPolicy(obs_dim)
    got, got_steps = agent.sample_trajectories_lockstep([_env(s, num_steps=n) for s, n in zip(seeds, lengths)], pol, batch_size=1,
                                                        max_trajectory_length=24)
    assert got_steps == want_steps
    _assert_same_paths(got, want)
    # one batched call per decision, finished environments dropped from the batch
    assert pol.calls == 0 and pol.batch_sizes[0] == 4 and pol.batch_sizes[-1] == 2      # (two end together at the max length)
    assert sorted(pol.batch_sizes, reverse=True) == pol.batch_sizes and len(set(pol.batch_sizes)) == 3
    assert sum(pol.batch_sizes) == sum(len(p['action']) for p in want)


def test_new_episodes_only_while_the_step_budget_lasts():
    obs_dim = _env(0).reset().shape[0]
    agent = _agent(1)
    envs = [_env(21, num_steps=10), _env(22, num_steps=10)]
    paths, steps = agent.sample_trajectories_lockstep(envs, BatchedLinearPolicy(obs_dim), batch_size=35, max_trajectory_length=50)
    # 2 x 10 steps after the first episodes (< 35: both restart), 40 after the second (>= 35: both stop)
    assert steps == 40 and len(paths) == 4
    assert all(len(p['action']) == 10 and p['terminal'][-1] == 1.0 for p in paths)
    # ordered by environment, then episode; each environment's two episodes are what two serial episodes of it are
    serial, _ = agent.sample_trajectories(_env(21, num_steps=10), LinearPolicy(obs_dim), batch_size=11, max_trajectory_length=50)
    _assert_same_paths(paths[:2], serial)
