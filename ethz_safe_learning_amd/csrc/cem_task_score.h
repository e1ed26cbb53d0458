// cem_task_score.h — the task scorer (cem_planner_set_task): quadratic rewards and box state constraints for plans whose
// observation is no Safety-Gym lidar vector.  A task plan runs the handle's MODE 1 rollout kernel unchanged, with RolloutParams::traj
// pointed at a buffer the handle owns; ONE kernel, this one, turns those trajectories and the candidates' actions into the `ret` and
// `costs` arrays the score, select, refit, keep and track kernels have always read (the rollout's own writes of the two are overwritten
// in stream order).  No rollout, sampler, reduce or select kernel changes, none reads what this one reads.
//
// THE CONTRACT (include/cem_mpc.h; planner.task_objective restates it in NumPy, bit for bit).  One row r of the rollout: states
// s_0 .. s_H raw and unscaled ([rows][H + 1][O], exactly what `traj` holds), actions a_0 .. a_{H-1} of candidate r mod N ([N][H][A]; the
// rows of a plan are p N + n, the reshape of mpc_policy.py:38).  Tables q, g, c, m, lo, hi [O] and rho [A]:
//   phi(s)  = sum_f [ q_f (s_f - g_f)^2 - c_f s_f ]
//   u(a)    = sum_j rho_j a_j^2
//   near(s) = R2 > 0 and sum_f m_f (s_f - g_f)^2 <= R2          R2 = fl32(goal_radius * goal_radius), rounded once on the host
//   viol(s) = 1.0 if any s_f < lo_f or s_f > hi_f, else 0.0      a NaN compares false
// and the bookkeeping of CEM_BOOKKEEP (cem_rollout_common.h), statement for statement, in both variant branches, with near(s_t) for
// `D_PREV <= goal_thresh`, -phi(s_{t+1}) - u(a_t) for `(D_PREV - dn) reward_distance` and viol(s_t) for C_PREV:
//   ga = near(s_t);  r = ((-phi(s_{t+1})) - u(a_t)) + (ga ? 1 : 0) * reward_goal;  r = fminf(fmaxf(r, -clip), clip)   (clip = +inf: none)
//   safe (safe_cem_mpc.py:86-93): done |= ga; nd = done ? 0 : 1; costs[t][r] = (uint8) (viol(s_t) * nd); cum += r * nd
//   cem  (mpc_policy.py:34-37):   nd = done ? 0 : 1; cum += r * nd; done |= ga            (no cost bytes)
// ret[r] = cum; a NaN is stored as the canonical quiet NaN 0x7fc00000 (a NaN's payload is no value: the host mirror stores the same).
//
// THE ARITHMETIC is fp32, every product and every sum rounded on its own (-ffp-contract=off), in ONE fixed order whatever the path:
//   per feature   d = s - g;  dd = d * d;  term = q * dd - c * s;  near term = m * dd
//   over features sixteen partial sums: partial l (0 .. 15) starts at +0 and adds the terms of features 64 i + 4 l + r, i = 0, 1 then
//                 r = 0 .. 3 (features >= O: tables q = c = m = 0 and s = g = 0, the term is +0); the sixteen are then added pairwise,
//                 neighbours first: (0 + 1), (2 + 3), ... then ((0 + 1) + (2 + 3)), ... four levels.  phi and the near sum alike.
//   over actions  u starts at +0 and adds rho_j * (a_j * a_j), j = 0 .. A - 1
//   over steps    t = 0 .. H - 1 as written above.
// The comparisons of near and viol are made on the ordered integer keys of the selects (cem_bits2key: the two zeros tie) behind a bit
// test for NaN, so -fno-honor-nans cannot change them.
//
// THE SHAPE is the task tile's (cem_task_tile.h states it once for the three kinds): this kernel is cem_task_rows of kind
// CEM_TASK_KIND_QUADRATIC — g from its table row, rho in the kernel arguments, no reference, clock or zone is read.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_score.hip defines
// CEM_TASK_SCORE_UNIT), as cem_plan_readout.h's is, so that the device code of cem_capi.hip stays what it was instruction for instruction.
#pragma once
#include "cem_task_tile.h"

// Weak: a library built from cem_capi.hip alone has no task scorer and cem_planner_set_task says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_score(const TaskParams &p, hipStream_t st);

#ifdef CEM_TASK_SCORE_UNIT
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_score_kernel(const TaskParams p) { cem_task_rows<NT, VEC, CEM_TASK_KIND_QUADRATIC>(p); }

hipError_t launch_task_score(const TaskParams &p, hipStream_t st)
{
    static const cem_task_kernel_t k[2][2] = {{cem_task_score_kernel<1, false>, cem_task_score_kernel<1, true>}, {cem_task_score_kernel<2, false>, cem_task_score_kernel<2, true>}};
    return cem_task_launch<CEM_TASK_KIND_QUADRATIC>(k, p, st);
}
#endif
