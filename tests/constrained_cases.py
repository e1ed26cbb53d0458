"""Budget-constrained planning (cem_mpc.h: cem_planner_set_constraint, CEM_CONSTRAINT_BUDGET) restated in NumPy, the
problems its tests share, a hand-written case and the table of shapes.  The reference has no such rule (constrained CEM: Wen & Topcu
2018); the definition in cem_mpc.h is the contract.

Everything here works on the handle's OWN returns [P, N] and cost bytes [H, P, N] of a rollout, so the device's scores must equal the
restatement bit for bit: integer sums, one fp32 division, one fp32 comparison, cem_reduce_kernel's sequential particle mean and an
exact encoding."""
import dataclasses

import numpy as np

from oracle import cem_oracle as o
from tests import cost_cases as cc
from tests import helpers as hp

TWO23 = 1 << 23


def encode_infeasible(total):
    """-(float)(2^23 + T) * 2^77 for integer T in [0, 2^23): exact, strictly decreasing in T, at or below -2^100."""
    t = np.asarray(total, np.int64)
    assert ((0 <= t) & (t < TWO23)).all()
    return -((t + TWO23).astype(np.float32)) * np.float32(2.0 ** 77)


def particle_costs(costs_u8, P, N):
    """cost bytes [H, P, N] -> c_p [P, N], integers."""
    c = np.asarray(costs_u8)
    assert c.ndim == 3 and c.shape[1:] == (P, N)
    return c.astype(np.int64).sum(axis=0)


def totals(costs_u8, P, N, m_c):
    """T [N]: the sum of the m_c largest per-particle cumulative costs (an integer sum: ties do not matter)."""
    assert 1 <= m_c <= P
    cp = np.sort(particle_costs(costs_u8, P, N), axis=0)[::-1]
    return cp[:m_c].sum(axis=0)


def cost_stats(costs_u8, P, N, m_c):
    """C [N] = (float)T / (float)m_c, one fp32 division."""
    return totals(costs_u8, P, N, m_c).astype(np.float32) / np.float32(m_c)


def mean_returns(returns):
    """cem_reduce_kernel's particle mean: particles q = 0 .. P-1 added in that order in fp32 from 0, divided once by P."""
    r = np.asarray(returns, np.float32)
    s = np.zeros(r.shape[1], np.float32)
    for q in range(r.shape[0]):
        s = s + r[q]
    return s / np.float32(r.shape[0])


def feasible(costs_u8, P, N, m_c, budget):
    return cost_stats(costs_u8, P, N, m_c) <= np.float32(budget)


def scores(returns, costs_u8, P, N, m_c, budget):
    """The handle's scores [N]: the mean return where C <= budget (fp32, inclusive), the encoded total elsewhere."""
    return np.where(feasible(costs_u8, P, N, m_c, budget), mean_returns(returns), encode_infeasible(totals(costs_u8, P, N, m_c))).astype(np.float32)


def decode(score):
    """(feasible, T or None) of one score."""
    s = np.float32(score)
    if s > np.float32(-2.0 ** 100):
        return True, None
    return False, int(-s * np.float32(2.0 ** -77)) - TWO23


def top_k(sc, k):
    """Indices of the k best scores, ties to the lowest index, ascending."""
    return np.sort(np.argsort(-np.asarray(sc, np.float64), kind='stable')[:k])


def constrained_elites(returns, costs_u8, P, N, m_c, budget, k):
    """The constrained-CEM elite set stated the long way: with at least k feasible candidates the k best-returning feasible ones,
    otherwise every feasible one and then the cheapest infeasible ones (by T; ties to the lowest index)."""
    f = feasible(costs_u8, P, N, m_c, budget)
    R, T = mean_returns(returns), totals(costs_u8, P, N, m_c)
    feas = [i for i in np.argsort(-R.astype(np.float64), kind='stable') if f[i]]
    infeas = [i for i in np.argsort(T, kind='stable') if not f[i]]
    return np.sort(np.array((feas + infeas)[:k]))


def plan(state, low, high, eps_act, eps_out, cfg, score_fn):
    """The CEM loop of CemMpc.do_generate_action (cem_mpc.py:35-68) on scores handed in by score_fn(it, actions) — the device's own —,
    as cost_cases.plan_cost runs it.  -> (action, best score, iterations)."""
    return cc.plan_cost(state, None, None, None, low, high, eps_act, None, eps_out, cfg, None, score_fn=score_fn)


def problem(E=5, seed=31, size_frac=1.0, **kw):
    """cost_cases.problem: costs that vary from the first step on."""
    return cc.problem(E=E, seed=seed, size_frac=size_frac, **kw)


def configs(pb, constraint='budget', worst_cost=0, **kw):
    ocfg, pcfg = hp.configs(pb, variant='safe', **kw)
    return ocfg, dataclasses.replace(pcfg, constraint=constraint, worst_cost_particles=worst_cost)


# name: P, N, H, E, size_frac.  P below, at and above the 16 waves of the kernel (1, 5 | 16 | 17, 45: one, two and three particles a wave)
# and the shipped 45; N = 70: a partial last block, 130: three blocks; H P = 3 .. 561: on both sides of one trip of 256 rows of the mean
# form; H below, at and above the 16 / J steps a trip of the tail form takes; E divides P N.
# size_frac (cost_cases.problem: the hazard sizes as a fraction of the start state's distances) is 1.0 where that splits the candidates
# for every m_c of risk_cases.tail_ms(P) at the median cost statistic, and smaller where at 1.0 every candidate's worst particles cost at
# every step (C = H for all of them).  Read off the fp32 ORACLE's first iteration with noise seed 5: candidates at or below the median,
# per m_c — p1: 36 of 70; p5_n130_h8 (0.7): 71, 77, 95, 95 of 130; p5_n70_h33: 36, 35, 37, 39 of 70; p16 (0.85): 45, 39, 37, 37 of 70;
# p17_n130_h33: 89, 72, 65, 65 of 130; p17_n70_h8 (0.7): 58, 60, 37, 37 of 70; p45_n70_h8 (0.7): 57, 58, 37, 37 of 70; p45_n130_h3
# (0.7): 76, 76, 68, 68 of 130.  The tests assert on the device's own bytes that both classes occur.
# P = 65 and 128: from five to eight particles a wave, the widest body of the tail form (the smallest P that takes it; H = 3 and 17: one
# trip of two steps and nine of them; and the cap CEM_BUDGET_MAX_TAIL_P, 36 KiB of LDS).  p65_n70_h3 (0.65; at 0.7 the worst particle
# of all 70 candidates sits at the median): 49, 49, 40, 40 of 70; p65_n70_h17 (0.7): 37, 37, 38, 38 of 70; p128_n70_h3 (0.7): 65, 66,
# 40, 40 of 70.
SHAPES = {
    'p1_n70_h3': (1, 70, 3, 5, 1.0),
    'p5_n130_h8': (5, 130, 8, 5, 0.7),
    'p5_n70_h33': (5, 70, 33, 5, 1.0),
    'p16_n70_h17': (16, 70, 17, 4, 0.85),
    'p17_n130_h33': (17, 130, 33, 5, 1.0),
    'p17_n70_h8': (17, 70, 8, 5, 0.7),
    'p45_n70_h8': (45, 70, 8, 15, 0.7),
    'p45_n130_h3': (45, 130, 3, 5, 0.7),
    'p65_n70_h3': (65, 70, 3, 5, 0.65),
    'p65_n70_h17': (65, 70, 17, 5, 0.7),
    'p128_n70_h3': (128, 70, 3, 4, 0.7),
}
NOISE_SEED = 5

# ---- the hand-written case: 3 particles x 4 candidates, 3 steps, budget 1 -------------------------------------------------------
HAND_P, HAND_N, HAND_H, HAND_BUDGET = 3, 4, 3, 1.0
# cost bytes [H, P, N].  Per-particle cumulative costs c_p:
#   candidate 0: 1, 1, 1   T = 3 over all, C = 1.0: exactly ON the budget (<= is inclusive); its worst particle costs 1: on it too
#   candidate 1: 0, 0, 3   T = 3 as well (the pair with equal T); the mean 1.0 is feasible, the worst particle (3) is not
#   candidate 2: 2, 1, 2   T = 5, C = 1.667: infeasible on the mean and on the worst particle (2)
#   candidate 3: 0, 0, 0   free
HAND_COSTS = np.zeros((HAND_H, HAND_P, HAND_N), np.uint8)
HAND_COSTS[0, 0, 0] = HAND_COSTS[1, 1, 0] = HAND_COSTS[2, 2, 0] = 1
HAND_COSTS[:, 2, 1] = 1
HAND_COSTS[0:2, 0, 2] = 1; HAND_COSTS[0, 1, 2] = 1; HAND_COSTS[0, 2, 2] = 1; HAND_COSTS[2, 2, 2] = 1
HAND_RETURNS = np.array([[1., 2., 5., .5],
                         [1., 2., 5., .25],
                         [1., 2.5, 5., 0.]], np.float32)                # means 1, 6.5 / 3, 5 (the best return, never feasible), 0.25
HAND_PARTICLE_COSTS = np.array([[1, 0, 2, 0], [1, 0, 1, 0], [1, 3, 2, 0]])
HAND_TOTALS = {3: np.array([3, 3, 5, 0]), 2: np.array([2, 3, 4, 0]), 1: np.array([1, 3, 2, 0])}
_R1 = np.float32(6.5) / np.float32(3)


def _enc(t):
    return np.float32(-(TWO23 + t) * 2.0 ** 77)                        # exact in float64, and in fp32 (an integer below 2^24 times a power of two)


HAND_SCORES = {3: np.array([1., _R1, _enc(5), .25], np.float32),
               2: np.array([1., _enc(3), _enc(4), .25], np.float32),
               1: np.array([1., _enc(3), _enc(2), .25], np.float32)}
# the same cost bytes as a trajectory for cem_compute_objective: obs = [goal lidar bin, hazard lidar bin, ...], cost_cases.HAND_SP
# (lidar_max_dist 1: a bin's value IS the distance; hazard size 0.25; goal reached below 0.4).  Rows p N + n; no row ever reaches the
# goal (bins 0.5 .. 0.9375, dyadic), so nothing is masked; the state after the last step is not scored for cost.
HAND_SP = cc.HAND_SP


def hand_trajectory(obs_dim):
    rows = HAND_P * HAND_N
    traj = np.full((rows, HAND_H + 1, obs_dim), 0.9, np.float32)
    for p in range(HAND_P):
        for n in range(HAND_N):
            r = p * HAND_N + n
            for t in range(HAND_H + 1):
                traj[r, t, 0] = 0.5 + ((5 * r + 3 * t) % 8) / 16.0
                traj[r, t, 1] = 0.125 if t < HAND_H and HAND_COSTS[t, p, n] else 0.875
    return traj
