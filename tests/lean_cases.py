"""The lean one-chunk rollout (csrc/cem_rollout_lean.hip) at its edges: the case table tests/test_gpu_lean_edges.py runs on the device
and tests/test_lean_cases_cpu.py checks on the host.  Plain data and small helpers; importable without a GPU or torch.

A case names a shape of the obs + act <= 64 family, the tile / segment plan it asks for, the action Box, the scorer and the rollout
path `lean_eligible` (cem_capi.hip) must give it.  Every case runs chunks_per_tile = 1 and units 128, E = P, k = max(2, N // 10).
What each group is there for:
  horizon      the two-steps-per-round loop and its `break`: H = 1 (tn = H - 1 = 0, the scratch slot H), H = 2, a segment resumed at an
               odd step (5 = 3 + 2), a short last segment (7 = 3 + 3 + 1), pinned and floating tiles in one launch
  lds_edge     (H + 1) ceil(A / 4) 304 bytes against the 16 KB allowance, one step either side, for 1, 2 and 8 action quads
  quads        action quads in two waves (obs 28: quad 7 in wave 1, quad 8 in wave 2), six and eight quads, obs + act = 64, act 1 of obs 4
  box          per-dimension asymmetric bounds (every quad holds other bounds; one dimension a single point), an unbounded Box and a
               Box with one infinite bound (the +-100 / 0 / 100 branch)
  scorer       every branch of hp.SCORER_CASES on obs 60, both objectives, unsegmented and in three segments (the done / d_prev /
               c_prev / cum quad then crosses two hand-overs)
  ineligible   depth 3 and obs 58: generic on both sides, the comparison still runs"""
import collections

import numpy as np

from tests import helpers as hp

INF = np.inf

# cem_rollout_lean.h: CEM_LEAN_ACT_LDS_BYTES(H, AZ) = (H + 1) AZ (32 + 17 * 16) and CEM_LEAN_ACT_LDS_MAX
LDS_BYTES_PER_QUAD_STEP = 32 + 17 * 16
LDS_MAX = 16384

# the plan every case starts (tests/test_gpu_lean_rollout.py: _run) and the problem seed of the scorer cases
PLAN_SEED, PLAN_CALL = 5, 3
SCORER_SEED = 31

Case = collections.namedtuple('Case', 'name group obs act E N H I segments variant box scorer depth path plan')
# plan: (segments, steps per segment) planner.plan_segments must return


def act_lds_bytes(H, A):
    return (H + 1) * ((A + 3) // 4) * LDS_BYTES_PER_QUAD_STEP


# name: (low, high) per dimension.  Mixed sign and width, no dimension the identity map (mu0 = 0, sigma0 = 1); asym6's dimension 4 (the
# first feature of the SECOND action quad) is a single point.
BOXES = {
    'asym3': ([-0.3, 0.5, -2.0], [1.7, 0.9, 0.25]),
    'asym6_one_point': ([-1.5, 0.25, -0.75, 1.0, 0.375, -3.0], [0.5, 0.75, 2.25, 1.5, 0.375, -1.0]),
    'asym8': (list(np.linspace(-2.0, 0.9, 8)), list(np.linspace(-1.5, 3.0, 8))),
    'asym24': (list(np.linspace(-2.0, 0.9, 24)), list(np.linspace(-1.5, 3.0, 24))),
    'unbounded2': ([-INF, -INF], [INF, INF]),
    'one_infinite2': ([-1.0, -0.5], [INF, 0.5]),                   # is_bounded() is False: +-100 for BOTH dimensions
}


def _cases():
    out = []

    def add(name, group, obs, act, N, H, I, segments, variant='cem', box=None, scorer=None, depth=4, E=2, path='lean'):
        seg_len = -(-H // segments)
        plan = (-(-H // seg_len), seg_len)
        out.append(Case(name, group, obs, act, E, N, H, I, segments, variant, box, scorer, depth, path, plan))

    # ---- horizon
    add('h1', 'horizon', 60, 2, 40, 1, 2, 1)
    add('h1_safe', 'horizon', 60, 2, 40, 1, 2, 1, 'safe')
    add('h2_two_segments', 'horizon', 60, 2, 40, 2, 2, 2)
    add('h5_resumed_at_an_odd_step', 'horizon', 60, 2, 40, 5, 2, 2)                 # 3 + 2
    add('h5_resumed_at_an_odd_step_safe', 'horizon', 60, 2, 40, 5, 2, 2, 'safe')
    add('h7_short_last_segment', 'horizon', 60, 2, 40, 7, 2, 3)                     # 3 + 3 + 1
    add('h7_short_last_segment_safe', 'horizon', 56, 6, 40, 7, 2, 3, 'safe')
    add('h7_pinned_and_floating', 'horizon', 60, 2, 2100, 7, 1, 3)                  # 264 tiles: 256 pinned + 8 floating
    # ---- the LDS allowance, one step either side
    add('lds_1quad_h52', 'lds_edge', 60, 2, 40, 52, 2, 1)                           # 16112 bytes
    add('lds_1quad_h53', 'lds_edge', 60, 2, 40, 53, 2, 1, path='generic')           # 16416
    add('lds_2quads_h25', 'lds_edge', 56, 6, 40, 25, 2, 1, 'safe')                  # 15808
    add('lds_2quads_h26', 'lds_edge', 56, 6, 40, 26, 2, 1, 'safe', path='generic')  # 16416
    add('lds_8quads_h5', 'lds_edge', 32, 32, 40, 5, 2, 1)                           # 14592
    add('lds_8quads_h6', 'lds_edge', 32, 32, 40, 6, 2, 1, path='generic')           # 17024
    add('lds_1quad_h52_four_segments', 'lds_edge', 60, 2, 40, 52, 2, 4, 'safe')     # 4 x 13: resumed at odd steps 13 and 39
    # ---- action quads
    add('quads_in_two_waves', 'quads', 28, 8, 40, 5, 2, 1)
    add('quads_in_two_waves_segmented', 'quads', 28, 8, 40, 5, 2, 2, 'safe')
    add('six_quads', 'quads', 40, 24, 40, 7, 2, 1)
    add('six_quads_segmented', 'quads', 40, 24, 40, 7, 2, 3)
    add('eight_quads_full_width', 'quads', 32, 32, 40, 4, 2, 2)
    add('full_quad_full_width', 'quads', 60, 4, 40, 5, 2, 1)
    add('act_1_of_obs_4', 'quads', 4, 1, 40, 5, 2, 1)
    add('act_1_of_obs_4_segmented', 'quads', 4, 1, 40, 5, 2, 2, 'safe')
    # ---- boxes
    add('box_asym3', 'box', 60, 3, 96, 5, 2, 1, box='asym3')
    add('box_asym3_segmented', 'box', 60, 3, 96, 5, 2, 2, 'safe', box='asym3')
    add('box_asym6_one_point', 'box', 56, 6, 96, 5, 2, 1, box='asym6_one_point')
    add('box_asym8_two_waves', 'box', 28, 8, 96, 5, 2, 1, box='asym8')
    add('box_asym8_two_waves_segmented', 'box', 28, 8, 96, 5, 2, 2, box='asym8')
    add('box_asym24', 'box', 40, 24, 96, 7, 2, 1, box='asym24')
    add('box_asym24_segmented', 'box', 40, 24, 96, 7, 2, 3, 'safe', box='asym24')
    add('box_unbounded', 'box', 60, 2, 96, 5, 2, 1, box='unbounded2')
    add('box_one_infinite_bound', 'box', 60, 2, 96, 5, 2, 2, box='one_infinite2')
    # ---- scorer branches
    for sc in hp.SCORER_CASES:
        for variant in ('cem', 'safe'):
            for segments in (1, 3):
                add('scorer_%s_%s_%dseg' % (sc, variant, segments), 'scorer', 60, 2, 96, 7, 2, segments, variant, scorer=sc)
    # ---- not eligible: generic on both sides
    add('depth_3', 'ineligible', 60, 2, 40, 3, 2, 1, depth=3, path='generic')
    add('obs_not_quad_aligned', 'ineligible', 58, 2, 40, 3, 2, 1, path='generic')
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
SCORER_CASES = [c for c in CASES if c.group == 'scorer']
BOX_CASES = [c for c in CASES if c.group == 'box']
# the LDS-edge pairs: (largest eligible horizon, first ineligible one)
LDS_PAIRS = [('lds_1quad_h52', 'lds_1quad_h53'), ('lds_2quads_h25', 'lds_2quads_h26'), ('lds_8quads_h5', 'lds_8quads_h6')]

_PROBLEMS = {}


def problem(case):
    """The case's synthetic problem (cached: weights and state are never written to)."""
    key = (case.obs, case.act, case.E, case.depth, case.box, case.scorer)
    if key not in _PROBLEMS:
        if case.scorer:
            assert (case.obs, case.act) == (60, 2)
            pb = hp.scorer_problem(case.scorer, case.obs, seed=SCORER_SEED, E=case.E)
        else:
            pb = hp.make_problem(case.obs, case.act, case.E, case.depth, seed=77)
        if case.box:
            pb = hp.with_action_bounds(pb, *BOXES[case.box])
        _PROBLEMS[key] = pb
    return _PROBLEMS[key]


def config_kwargs(case):
    """What hp.configs and tests/test_gpu_lean_rollout.py's _compare take for the case."""
    return dict(N=case.N, H=case.H, P=case.E, E=case.E, k=max(2, case.N // 10), I=case.I, variant=case.variant, post=0.3,
                chunks_per_tile=1, rollout_segments=case.segments)


def oracle_iteration0(case, eps_act0, eps_model0):
    """Iteration 0 of the case's plan in the fp64 oracle on the given streams (eps_act0 [N, H, A], eps_model0 [H, P N, O], fp32):
    -> (sampled actions fp32 [N, H, A], scores fp64 [N], trajectories fp64 [P N, H + 1, O])."""
    from oracle import cem_oracle as o
    pb = problem(case)
    ocfg, _ = hp.configs(pb, **config_kwargs(case))
    lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
    shape = (case.H, case.act)
    actions = o.sample_actions(np.broadcast_to(mu0, shape), np.broadcast_to(sg0, shape), lb, ub, np.asarray(eps_act0, np.float32))
    ref64, traj64 = o.candidate_scores(pb['state'].astype(np.float64), actions.astype(np.float64), o.cast_weights(pb['weights'], np.float64),
                                       pb['inputs_min'], pb['inputs_max'], np.asarray(eps_model0, np.float32), ocfg, pb['scorer'], return_traj=True)
    return actions, ref64, traj64


def masked_costs_and_first_goal(traj64, sp):
    """SafeCemMpc's per-step costs (safe_cem_mpc.py:89: done OR-ed first, then cost(s_t) (1 - done)) [H, rows], and per row the step at
    which the goal is first reached (H where it never is)."""
    from oracle import cem_oracle as o
    B, H = traj64.shape[0], traj64.shape[1] - 1
    done = np.zeros(B, bool)
    costs = np.zeros((H, B))
    first = np.full(B, H)
    for t in range(H):
        _, d = o.reward(traj64[:, t], traj64[:, t + 1], sp)
        first[d & ~done] = t
        done |= d
        costs[t] = o.cost(traj64[:, t], sp) * (1.0 - done)
    return costs, first
