"""The cost-minimising objective (enum cem_variant CEM_VARIANT_COST; SafeCemMpc.optimize_for_safety / compute_mean_costs,
reference simba/policies/safe_cem_mpc.py:40-74,98-108) restated in NumPy from the oracle's existing pieces, and the problems the tests
of it share.  The oracle itself has no cost objective."""
import dataclasses

import numpy as np

from oracle import cem_oracle as o
from tests import helpers as hp


def mean_cost_scores(traj, P, N, sp):
    """-compute_mean_costs (safe_cem_mpc.py:98-108, negated at :61): traj [P*N, H+1, O], rows p*N + n -> scores [N]."""
    dt = traj.dtype
    cum = np.zeros((traj.shape[0],), dt)                               # :99
    for t in range(traj.shape[1] - 1):                                 # :101  (horizon - 1 steps)
        cum = cum + o.cost(traj[:, t], sp)                             # :102-106  cost(s_t, a_t, s_t+1) looks at s_t alone; NO done mask
    per = cum.reshape(P, N)                                            # :107
    mean = (per.sum(axis=0, dtype=dt) / dt.type(P)).astype(dt)         # :108  reduce_mean over the particles
    return -mean                                                       # :61


def scores_from_bytes(costs_u8, P, N):
    """The same arithmetic on cost bytes [H, P, N] (the device's own): fp32 sums of small integers are exact, the division rounds once."""
    c = np.asarray(costs_u8).astype(np.float32)
    cum = c.sum(axis=0, dtype=np.float32)                              # :101-106
    return -(cum.reshape(P, N).sum(axis=0, dtype=np.float32) / np.float32(P))      # :107-108, :61


def cost_bytes(traj, sp):
    """cost of every (step, row): [H, B] (the layout of cem_layout_t::costs), in the trajectory's dtype."""
    return np.stack([o.cost(traj[:, t], sp) for t in range(traj.shape[1] - 1)])


def cost_margins(traj, sp):
    """[H, B]: the smallest |closest_distance - cost_size| over the constrained kinds — how close a step's cost is to flipping."""
    H = traj.shape[1] - 1
    m = np.full((H, traj.shape[0]), np.inf)
    for t in range(H):
        for lo, hi, size in sp.cost_kinds:
            m[t] = np.minimum(m[t], np.abs(o.closest_distance(traj[:, t, lo:hi].astype(np.float64), sp) - size))
    return m


def plan_cost(state, weights, inputs_min, inputs_max, low, high, eps_act, eps_model, eps_out, cfg, sp, score_fn=None, dtype=np.float32):
    """SafeCemMpc.optimize_for_safety (safe_cem_mpc.py:40-74): the loop of CemMpc.do_generate_action on mean_cost_scores.
    score_fn(it, actions) replaces the rollout + objective (the tests hand in the device's own scores).  -> (action, best score, iterations)."""
    dt = np.dtype(dtype).type
    A = np.asarray(low).shape[0]
    lb, ub, mu0, sigma0 = o.sampling_params(low, high, dtype)                               # :42
    mu = np.broadcast_to(mu0, (cfg.horizon, A)).astype(dtype).copy()                        # :44
    sigma = np.broadcast_to(sigma0, (cfg.horizon, A)).astype(dtype).copy()                  # :45
    best, best_score, iters = np.zeros((A,), dtype), dt(-np.inf), 0                         # :46-47
    members = o.member_of_rows(cfg.particles * cfg.n_samples, cfg.ensemble_size)
    for it in range(cfg.iterations):                                                        # :48
        actions = o.sample_actions(mu, sigma, lb, ub, eps_act[it].astype(dtype))            # :49-53
        if score_fn is not None:
            scores = score_fn(it, actions)
        else:
            s0 = np.broadcast_to(np.asarray(state, dtype), (cfg.particles * cfg.n_samples, np.shape(state)[0])).copy()
            traj = o.unfold_sequences(s0, np.tile(actions, (cfg.particles, 1, 1)), weights, members, inputs_min, inputs_max,
                                      eps_model[it].astype(dtype), cfg.scale_features, cfg.sampling_propagation)    # :54-59
            scores = mean_cost_scores(traj, cfg.particles, cfg.n_samples, sp)               # :60-61
        mu, sigma, best, best_score, _, stop = o.select_and_refit(scores, actions, mu, sigma, best, best_score, cfg)   # :62-71
        iters += 1
        if stop:                                                                            # :72-73
            break
    return best + np.asarray(eps_out, dtype) * dt(cfg.noise_stddev), best_score, iters      # :74


def problem(E=5, kinds=(1,), indicator=True, size_frac=1.0, seed=31, near_goal=False, **kw):
    """A synthetic problem whose cost is not constant: the constrained kinds' sizes are size_frac x the closest distance of the start
    state (1.0: predicted states drift in and out of them from the first step on).  near_goal: the start state's goal distance lies
    below goal_reached_dist, so the safe objective masks every step."""
    pb = hp.scorer_problem('four_kinds_sum', seed=seed, E=E)           # lidar-like values and a [0, 1] normaliser on every lidar slice
    if kw:                                                             # another network (units, activation) on the same state
        pb = dict(hp.make_problem(E=E, seed=seed, **kw), state=pb['state'], inputs_min=pb['inputs_min'], inputs_max=pb['inputs_max'])
    lay, sp = hp.SCORER_LAYOUTS[60], pb['scorer']
    ck = [(lay['kinds'][i][0], lay['kinds'][i][1],
           float(np.float32(size_frac * sp.lidar_max_dist * pb['state'][lay['kinds'][i][0]:lay['kinds'][i][1]].min()))) for i in kinds]
    if near_goal:
        pb['state'][lay['goal'][0]] = np.float32(0.03)                 # closest goal distance 0.12 <= 0.8 * 0.3
    pb['scorer'] = dataclasses.replace(sp, goal_slice=lay['goal'], observe_goal_lidar=True, constrain_indicator=indicator, cost_kinds=ck)
    return pb


def configs(pb, N, H, P, E, k, **kw):
    """(oracle config, planner config) of a cost handle (the oracle's PlanConfig has no such variant: it carries the loop's constants)."""
    ocfg, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=k, **kw)
    return ocfg, dataclasses.replace(pcfg, variant='cost')


# hand-written case of the restatement: 2 particles x 3 candidates, 3 steps (+ the final state), obs = [goal lidar bin, hazard lidar bin].
# lidar_max_dist 1: closest distance = the bin's value.  goal_size 0.5 -> reached below 0.4; hazard size 0.25.
HAND_SP = o.ScorerParams(goal_slice=(0, 1), observe_goal_lidar=True, lidar_max_dist=1.0, goal_size=0.5, reward_distance=1.0, reward_goal=1.0,
                         reward_clip=10.0, constrain_indicator=True, cost_kinds=[(1, 2, 0.25)])
_G = 0.1                                                               # every row has reached the goal at step 0
# hazard bin per (row, step 0..3): <= 0.25 costs 1.  Rows p*3 + n.
HAND_HAZ = np.array([[.2, .2, .9, .2],      # p0 n0: 1 1 0 (the state after the last step is not scored)
                     [.9, .9, .9, .1],      # p0 n1: 0 0 0
                     [.25, .9, .2, .9],      # p0 n2: 1 0 1  (<= is inclusive)
                     [.9, .2, .9, .9],      # p1 n0: 0 1 0
                     [.9, .9, .9, .9],      # p1 n1: 0 0 0
                     [.1, .1, .1, .9]],     # p1 n2: 1 1 1
                    np.float32)
HAND_TRAJ = np.stack([np.full_like(HAND_HAZ, _G), HAND_HAZ], axis=2)   # [6, 4, 2]
HAND_SCORES = np.array([-(2 + 1) / 2, -0.0, -(2 + 3) / 2], np.float32)
