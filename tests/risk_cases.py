"""The lower-tail particle objective (cem_mpc.h: cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL) restated
in NumPy, the small problems its tests share, and the table of shapes.  The reference has no such objective (its
random_shooting_mpc.py:11,35 takes an `objective` argument that nothing defines): the definition in cem_mpc.h is the contract.

Everything here works on the handle's OWN returns [P, N] and cost bytes [H, P, N] of a rollout, so the device's scores must equal the
restatement bit for bit: a stable sort, a sequential fp32 sum, one division, and cem_reduce_kernel's Beta filter."""
import dataclasses

import numpy as np

from oracle import cem_oracle as o
from tests import helpers as hp

O, A = 12, 2                     # obs [goal lidar 0:4 | hazards lidar 4:8 | 4 other], 2 layers of 32 units


def lower_tail_values(returns, m):
    """returns [P, N] -> [N]: particles ascending by (return, particle index), the first m added in that order in fp32 from 0, / m."""
    r = np.asarray(returns, np.float32)
    assert r.ndim == 2 and 1 <= m <= r.shape[0] and not np.isnan(r).any()
    order = np.argsort(r, axis=0, kind='stable')                       # equal returns (-0.0 == 0.0 too) stay in particle order
    srt = np.take_along_axis(r, order, axis=0)
    s = np.zeros(r.shape[1], np.float32)
    for i in range(m):
        s = s + srt[i]
    return s / np.float32(m)


def unsafe_flags(costs_u8, P, thr):
    """cost bytes [H, P, N] -> bool [N]: OR over steps of (alpha + count_t) / ((alpha + beta) + P) > thr (safe_cem_mpc.py:110-120)."""
    alpha, beta = o.beta_prior()
    cnt = np.asarray(costs_u8).astype(np.float32).sum(axis=1, dtype=np.float32)        # [H, N]; small integers: exact
    post = (alpha + cnt) / ((alpha + beta) + np.float32(P))
    return (post > np.float32(thr)).any(axis=0)


def scores(returns, m, costs_u8=None, thr=None):
    """The handle's scores: the lower-tail value; on a 'safe' handle (costs_u8 given) minus 100 where the Beta filter says unsafe."""
    v = lower_tail_values(returns, m)
    if costs_u8 is None:
        return v
    u = unsafe_flags(costs_u8, np.asarray(returns).shape[0], thr)
    return v - np.where(u, np.float32(1.0), np.float32(0.0)) * np.float32(100.0)


def top_k(sc, k):
    """Indices of the k best scores, ties to the lowest index, ascending."""
    return np.sort(np.argsort(-np.asarray(sc), kind='stable')[:k])


def tail_ms(P):
    """m in {1, 2, P - 1, P} where defined."""
    return sorted({m for m in (1, 2, P - 1, P) if 1 <= m <= P})


def problem(E=5, seed=41, size_frac=0.95, units=32, **kw):
    """A small synthetic problem whose hazard cost is not constant: the hazard size is size_frac x the closest hazard distance of the
    start state (0.95: the start state itself is outside), so predicted states drift in and out of it."""
    pb = hp.make_problem(obs_dim=O, act_dim=A, E=E, n_layers=2, units=units, seed=seed, **kw)
    sp = pb['scorer']
    (lo, hi, _), = sp.cost_kinds
    size = float(np.float32(size_frac * sp.lidar_max_dist * pb['state'][lo:hi].min()))
    pb['scorer'] = dataclasses.replace(sp, cost_kinds=[(lo, hi, size)])
    return pb


def configs(pb, worst=0, **kw):
    ocfg, pcfg = hp.configs(pb, **kw)
    return ocfg, dataclasses.replace(pcfg, worst_particles=worst)


# name: P, N, H, E, posterior threshold of the 'safe' handle.  P crosses the 16 waves of the kernel (1, 5 | 16 | 17, 45: one, two and three
# particles a wave) and includes the shipped 45; N = 70: a partial last block, 130: three blocks; H below and from 16 on: the two
# branches of the Beta count (33: a wave counts three steps); E divides P N.
# The thresholds: a candidate is unsafe when some step's count exceeds c, i.e. thr = (alpha + c + 0.5) / (2 alpha + P) with
# alpha = beta = 1.2147 (half a count away from either neighbour).  c was read off the fp32 ORACLE's per-candidate largest step count for
# problem() with noise seed 5 (the count histogram's middle: 30 of 70 candidates at or below c for p1, 91 of 130 for p5_n130_h8, ...), so
# that both safe and unsafe candidates occur; the tests assert that they do on the device's own bytes.
# P = 65 and 128: from five to eight particles a wave, the widest body of the ranking kernels (the smallest P that takes it, N no multiple
# of 64, on both branches of the Beta count; and the cap CEM_TAIL_MAX_P, 40 KiB of LDS).  Their c, read off the same way: 33 of 70 at or
# below 27 for p65_n70_h3 (0.4 P); 35 of 70 at or below 41 for p65_n70_h17 and at or below 59 for p128_n70_h3, whose smallest counts
# are 38 and 52 (at 0.4 P every candidate of either would be unsafe).
def _thr(P, c):
    return round((1.2147 + c + 0.5) / (2 * 1.2147 + P), 4)


SHAPES = {
    'p1_n70_h3': (1, 70, 3, 5, _thr(1, 0)),
    'p5_n130_h8': (5, 130, 8, 5, _thr(5, 3)),
    'p5_n70_h33': (5, 70, 33, 5, _thr(5, 3)),
    'p16_n70_h17': (16, 70, 17, 4, _thr(16, 12)),
    'p17_n130_h33': (17, 130, 33, 5, _thr(17, 11)),
    'p17_n70_h8': (17, 70, 8, 5, _thr(17, 9)),
    'p45_n70_h8': (45, 70, 8, 15, _thr(45, 19)),
    'p45_n130_h3': (45, 130, 3, 5, _thr(45, 19)),
    'p65_n70_h3': (65, 70, 3, 5, _thr(65, 27)),
    'p65_n70_h17': (65, 70, 17, 5, _thr(65, 41)),
    'p128_n70_h3': (128, 70, 3, 4, _thr(128, 59)),
}
NOISE_SEED = 5

# hand-written arrays: 5 particles x 4 candidates
HAND_RETURNS = np.array([[9., -1., 2., 0.],
                         [9., -1., 2., -0.],
                         [9., -1., -3., 5.],
                         [9., -1., 2., 0.],
                         [-40., -1., -3., -7.]], np.float32)
# candidate 0: the issue's [9, 9, 9, 9, -40]; 1: all equal; 2: ties in the tail (-3 twice, 2 three times); 3: signed zeros tie
HAND_TAIL = {1: np.array([-40., -1., -3., -7.], np.float32),
             2: np.array([(-40. + 9.) / 2, -1., -3., -3.5], np.float32),
             4: np.array([(-40. + 27.) / 4, -1., -0.5, -1.75], np.float32),
             5: np.array([np.float32(-4.) / np.float32(5.), -1., 0., np.float32(-2.) / np.float32(5.)], np.float32)}
# cost bytes [H = 2, P = 5, N = 4]: candidate 1 costs on 4 of 5 particles at step 1, candidate 3 on 2 of 5 at step 0, the others never
HAND_COSTS = np.zeros((2, 5, 4), np.uint8)
HAND_COSTS[1, :4, 1] = 1
HAND_COSTS[0, :2, 3] = 1
# alpha = beta = 1.2147..: posterior means (alpha + c) / (2 alpha + 5) = 0.1635 (c = 0), 0.4327 (c = 2), 0.7019 (c = 4)
HAND_UNSAFE = {0.5: np.array([False, True, False, False]), 0.3: np.array([False, True, False, True]), 0.1: np.ones(4, bool)}
