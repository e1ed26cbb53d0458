// cem_task_zones.h — keep-out and keep-in zones on a task (cem_planner_set_task_zones): up to CEM_TASK_MAX_ZONES
// axis-aligned ellipsoids on up to CEM_TASK_ZONE_AXES state features each, which a plan must stay out of (hazards, pillars) or inside
// of.  A zone that is hit sets the step's cost byte exactly as the box does; a zone that is near costs reward through a hinge.  A task
// plan with zones launches what its base task plan launches, with ONE kernel, this one, in the place of cem_task_score_kernel /
// cem_task_reference_kernel.  A task without zones never comes here.
//
// THE CONTRACT (include/cem_mpc.h; planner.task_objective / tracking_objective restate it in NumPy, bit for bit).  Everything not named
// here is cem_task_reference.h's, statement for statement; a quadratic base task is the tracking task with one reference row g, qT = q,
// kappa = 0 and the clock at (0, zeros).  Zone z: axes axis[z][d] (-1: slot unused), centre c[z][d], weights w[z][d], R2 = fl32(radius^2),
// Rm2 = fl32((radius + margin)^2) (keep-in: (radius - margin)^2), both rounded once on the host, penalty, keep_in.  For state s:
//   dist2 starts at +0; d = 0 .. 3 with a used axis:  e = s[axis] - c;  dist2 = dist2 + w * (e * e)      every operation rounded on its own
//   keep-out: hit = dist2 <= R2;  hinge = fmaxf(Rm2 - dist2, 0)        keep-in: hit = dist2 > R2;  hinge = fmaxf(dist2 - Rm2, 0)
//   a NaN dist2 hits nothing and its hinge is +0; the comparisons are made on the selects' integer keys behind the NaN bit test
//   pen(s): sixteen slots, slot z = penalty_z * hinge_z (z >= n_zones: +0), added pairwise, neighbours first, four levels
//   viol(s) = the box's viol(s) or any hit_z(s)
//   r = ((((-phi(s_{t+1})) - u(a_t)) - v_t) - pen(s_{t+1})) + (ga ? 1 : 0) * reward_goal;  the clip and the variant branches unchanged.
//
// THE SHAPE is the task tile's (cem_task_tile.h): this kernel is cem_task_rows of kind CEM_TASK_KIND_ZONES, the tracking kind's body
// with the zones' statements switched in, and the sixteen lanes that own a row own one zone each: lane l evaluates zone l on the
// state its group has just loaded.  Its <= 4 axis features are element loads of the same state, requested in the same batch as the
// state's quads (they hit the lines those fetch: no second read of `traj` from memory).  `hit` joins the box test in front of the one
// ballot, `pen` goes through the four shuffles phi and the near sum go through.  The zone table is a device allocation of the handle's,
// sixteen words a zone (CEM_TASK_ZONE_WORDS): a lane reads its zone's four 16-byte rows once, in front of the loop.  No LDS, no atomics.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_zones.hip defines
// CEM_TASK_ZONES_UNIT) and holds that kernel alone: a library without the unit has no zones, and the unit's recorded resources
// (tests/golden/task_zones_resources.json) are this kernel's.
#pragma once
#include "cem_task_tile.h"

// Weak: a library built without cem_task_zones.hip has no zones and cem_planner_set_task_zones says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_zones(const TaskParams &p, hipStream_t st);

#ifdef CEM_TASK_ZONES_UNIT
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_zones_kernel(const TaskParams p) { cem_task_rows<NT, VEC, CEM_TASK_KIND_ZONES>(p); }

hipError_t launch_task_zones(const TaskParams &p, hipStream_t st)
{
    static const cem_task_kernel_t k[2][2] = {{cem_task_zones_kernel<1, false>, cem_task_zones_kernel<1, true>}, {cem_task_zones_kernel<2, false>, cem_task_zones_kernel<2, true>}};
    return cem_task_launch<CEM_TASK_KIND_ZONES>(k, p, st);
}
#endif
