// cem_task_outputs.h — linear outputs on a task (cem_planner_set_task_outputs): up to CEM_TASK_MAX_OUTPUTS derived
// features y = C s of the state, each with the task's whole vocabulary — weight, target or per-step reference, linear term, near-goal
// weight, box bound, terminal weight, zone axis.  Q = L^T L states a full-matrix cost with C = L; a bound on an output is a half-space,
// M bounded outputs a polytope; two outputs under a rotation carry a rotated ellipse.  A task plan with outputs launches what its base
// task plan launches, with ONE kernel, this one, in the place of cem_task_score_kernel / cem_task_reference_kernel /
// cem_task_zones_kernel.  A task without outputs never comes here.
//
// THE CONTRACT (include/cem_mpc.h; planner.output_terms, task_objective and tracking_objective restate it in NumPy, bit for bit).
// Everything not named here is cem_task_zones.h's, statement for statement, with n_zones = 0 allowed.  M = n_outputs, C [M][O]; a state
// has features 0 .. O - 1 and outputs O .. O + M - 1.  For state s and output m:
//   y_m: sixteen partials; partial l starts at +0 and adds C[m][f] * s_f for f = 64 i + 4 l + r, i = 0, 1 and then r = 0 .. 3 (the
//        features lane l owns; those >= O add nothing); the sixteen are added pairwise, neighbours first, four levels (phi's tree)
//   e = y_m - gy_m (a tracking base: gy is row min(k0 + st, T - 1) of the outputs' reference when that has T rows);  ee = e * e
//   w = terminal ? qTy_m : qy_m;   phi's partial m += (w * ee - cy_m * y_m), behind that partial's feature terms;   near's partial m += my_m * ee
//   viol(s) also ORs in y_m < loy_m or y_m > hiy_m (a NaN compares false; on the selects' keys behind the NaN bit test)
//   a zone axis O + m reads y_m where it read s[axis]; the zone's arithmetic is unchanged
// Every product, difference and sum is rounded on its own (-ffp-contract=off).  A partial that starts at +0 never becomes -0, so an
// idle output (qy = qTy = cy = my = 0, infinite bounds) adds (+0 - +-0) = +0 to it and leaves the bits of the task without outputs.
//
// THE SHAPE is the task tile's (cem_task_tile.h): this kernel is cem_task_rows of kind CEM_TASK_KIND_OUTPUTS, the zones kind's body with
// the outputs' statements switched in.  C sits in LDS (8 KB, the tile's only LDS, copied once per block): sixteen more quads per lane
// do not fit beside the zones kind's registers.  Lane l reads its quad of row m with one 16-byte LDS load and uses it for all
// CEM_TASK_DEPTH states in flight; a row from n_outputs on is skipped.  The sixteen dot products of a state meet through a butterfly
// reduce-scatter over xor distances 1, 2, 4, 8 — at distance d a lane keeps the outputs whose bit d is its own: 15 exchanges, not 64 —
// and lane l ends holding exactly y_l, as the sixteen lanes own one zone each.  A zone lane fetches an output it names with one
// variable-source lane read.  `traj` is still read once.  No atomics, no scratch.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_outputs.hip defines
// CEM_TASK_OUTPUTS_UNIT) and holds that kernel alone: a library without the unit has no outputs, and the unit's recorded resources
// (tests/golden/task_outputs_resources.json) are this kernel's.
#pragma once
#include "cem_task_tile.h"

// Weak: a library built without cem_task_outputs.hip has no outputs and cem_planner_set_task_outputs says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_outputs(const TaskParams &p, hipStream_t st);

#ifdef CEM_TASK_OUTPUTS_UNIT
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_outputs_kernel(const TaskParams p) { cem_task_rows<NT, VEC, CEM_TASK_KIND_OUTPUTS>(p); }

hipError_t launch_task_outputs(const TaskParams &p, hipStream_t st)
{
    static const cem_task_kernel_t k[2][2] = {{cem_task_outputs_kernel<1, false>, cem_task_outputs_kernel<1, true>}, {cem_task_outputs_kernel<2, false>, cem_task_outputs_kernel<2, true>}};
    return cem_task_launch<CEM_TASK_KIND_OUTPUTS>(k, p, st);
}
#endif
