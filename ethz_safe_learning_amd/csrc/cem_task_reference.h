// cem_task_reference.h — the tracking task (cem_planner_set_task_tracking): the quadratic task of cem_task_score.h with a
// set-point that moves with time, a weight of its own on the last predicted state and a penalty on how fast the action changes.  A
// tracking plan launches what a quadratic-task plan launches, with ONE kernel, this one, in the place of cem_task_score_kernel.
//
// THE CONTRACT (include/cem_mpc.h; planner.tracking_objective restates it in NumPy, bit for bit).  Everything not named here is
// cem_task_score.h's, statement for statement.  Tables q, c, m, lo, hi [O] and rho [A] as there; qT [O] (default q), kappa [A] (default
// 0), ref [T][O] with 1 <= T <= CEM_TASK_REF_MAX_STEPS; the clock (k0 >= 0, a_{-1} [A]).  For state s_st, st = 0 .. H:
//   j = min(k0 + st, T - 1)                       the reference row: the last row is held
//   d = s - ref[j];  dd = d * d;  term = w * dd - c * s  with w = qT where st == H, else q;  near term = m * dd
// the lane partials and the pairwise tree as there.  The action-rate term of step t starts at +0 and adds, j = 0 .. A - 1,
//   e = a_t[j] - a_{t-1}[j]  (a_{-1}: the clock's);  v = v + kappa_j * (e * e)          every operation rounded on its own
// and the reward is  r = (((-phi(s_{t+1})) - u(a_t)) - v_t) + (ga ? 1 : 0) * reward_goal;  the clip, the variant branches, the NaN
// canonicalisation and the key comparisons follow unchanged.  With T = 1, ref[0] = g, qT = q and kappa = 0 the result is
// cem_task_score_kernel's bit for bit (x - (+0) is x).
//
// THE SHAPE is the task tile's (cem_task_tile.h): this kernel is cem_task_rows of kind CEM_TASK_KIND_TRACKING, the same body as
// cem_task_score_kernel with the statements above switched in.  The reference table is a device allocation of the
// handle's: row stride CEM_U floats, zero beyond O, 16-byte aligned — so a lane's reference quad is ONE 16-byte load whatever O is,
// requested with the state loads of the same batch (the table is a few KB to 8 MB: it stays in L2).  q, qT, c, m and the lo / hi keys sit
// in registers, rho and kappa in the kernel arguments.  k0 and a_{-1} are read from DEVICE MEMORY (the clock block: word 0 is k0, words
// 1 .. A are a_{-1}), never from the kernel arguments: a captured plan sees the clock that cem_planner_set_task_clock's stream-ordered
// copy left.  No LDS, no atomics.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_reference.hip defines
// CEM_TASK_REFERENCE_UNIT), as cem_task_score.h's is, and holds that kernel alone: a library without the unit has no tracking task, and
// the unit's recorded resources (tests/golden/task_reference_resources.json) are this kernel's.
#pragma once
#include "cem_task_tile.h"

// Weak: a library built without cem_task_reference.hip has no tracking task and cem_planner_set_task_tracking says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_reference(const TaskParams &p, hipStream_t st);

#ifdef CEM_TASK_REFERENCE_UNIT
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_reference_kernel(const TaskParams p) { cem_task_rows<NT, VEC, CEM_TASK_KIND_TRACKING>(p); }

hipError_t launch_task_reference(const TaskParams &p, hipStream_t st)
{
    static const cem_task_kernel_t k[2][2] = {{cem_task_reference_kernel<1, false>, cem_task_reference_kernel<1, true>}, {cem_task_reference_kernel<2, false>, cem_task_reference_kernel<2, true>}};
    return cem_task_launch<CEM_TASK_KIND_TRACKING>(k, p, st);
}
#endif
