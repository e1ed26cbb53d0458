"""BaseAgent's warm-start hooks, with stand-in policies (no GPU): sample_trajectory resets a policy that has a reset(), the lockstep
sampler tells a slot-aware policy which environment every row belongs to and which rows begin an episode, and policies without the hooks
are called exactly as before."""
import numpy as np

from ethz_safe_learning_amd.simba.agents.agent import BaseAgent
from ethz_safe_learning_amd.simba.spaces import Box


class _Env:
    def __init__(self, length):
        self.length, self.t, self.episodes = length, 0, 0
        self.action_space = Box(-np.ones(2, np.float32), np.ones(2, np.float32))

    def reset(self):
        self.t = 0
        self.episodes += 1
        return np.full(3, self.episodes, np.float32)

    def step(self, action):
        self.t += 1
        return np.full(3, self.episodes + self.t / 100, np.float32), 1.0, self.t >= self.length, {}


class _SlotPolicy:
    accepts_slots = True

    def __init__(self):
        self.calls, self.resets = [], 0

    def reset(self):
        self.resets += 1

    def generate_action(self, obs):
        return np.zeros(2, np.float32)

    def generate_actions(self, states, slots=None, reset=None):
        self.calls.append((len(states), list(map(int, slots)), list(map(bool, reset))))
        return np.zeros((len(states), 2), np.float32)


class _PlainBatchPolicy:
    def __init__(self):
        self.calls = []

    def generate_actions(self, states):                      # no slots / reset parameters: must be called without them
        self.calls.append(len(states))
        return np.zeros((len(states), 2), np.float32)


def _agent():
    return BaseAgent(replay_buffer_size=100, add_observation_noise=False, action_repeat=1)


def test_sample_trajectory_resets_a_policy_that_can_be_reset():
    pol = _SlotPolicy()
    _agent().sample_trajectories(_Env(3), pol, batch_size=9, max_trajectory_length=10)
    assert pol.resets == 3                                    # one per episode


def test_lockstep_passes_environment_indices_and_episode_starts():
    pol = _SlotPolicy()
    envs = [_Env(2), _Env(4), _Env(3)]
    paths, steps = _agent().sample_trajectories_lockstep(envs, pol, batch_size=8, max_trajectory_length=10)
    assert steps == 2 + 2 + 4 + 3 and len(paths) == 4
    # decision 1: all start; 2: none; 3: environment 0 ended after 2 steps and restarts (steps = 6 < 8); then rows compact as episodes end
    assert pol.calls[0] == (3, [0, 1, 2], [True, True, True])
    assert pol.calls[1] == (3, [0, 1, 2], [False, False, False])
    assert pol.calls[2] == (3, [0, 1, 2], [True, False, False])
    assert pol.calls[3] == (2, [0, 1], [False, False])        # environment 2 ended at step 9 >= batch_size and dropped out
    for n, slots, reset in pol.calls:
        assert n == len(slots) == len(reset) and len(set(slots)) == n


def test_policies_without_the_hooks_are_called_as_before():
    pol = _PlainBatchPolicy()
    _agent().sample_trajectories_lockstep([_Env(2), _Env(3)], pol, batch_size=4, max_trajectory_length=10)
    assert pol.calls and all(isinstance(n, int) for n in pol.calls)
