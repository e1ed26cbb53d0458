// cem_rollout_lean.h — what cem_capi.hip knows of the lean one-chunk rollout (cem_rollout_lean.hip, a translation unit of its own).
#pragma once
#include "cem_device.h"

// Dynamic LDS of the lean kernels: the generic one-chunk tile's, then the plan's mu / sigma of every step and the action bounds as
// zero-padded quads, [H][ceil(A / 4)] {sigma, mu} and [ceil(A / 4)] {lb, ub} (B2: 960 + 32 bytes), then the parking area of the sampled
// actions, [16 rows + 1][H + 1][ceil(A / 4)] quads (B2: 8432 bytes).
#define CEM_LEAN_ACT_LDS_BYTES(H_, AZ_) (((size_t)(H_) + 1) * (AZ_) * (32 + 17 * 16))
#define CEM_LEAN_LDS_BYTES(H_, AZ_) (CEM_ROLLOUT_LDS_BYTES(1) + CEM_LEAN_ACT_LDS_BYTES(H_, AZ_))
// the most of it a handle may ask for and still keep the generic kernel's three workgroups per CU by a wide margin (else: generic path)
#define CEM_LEAN_ACT_LDS_MAX 16384

// grid workgroups of cem_rollout_lean_kernel (seg false: one per tile) or cem_rollout_lean_seg_kernel (seg true: pinned tiles, then one per
// (floating tile, segment) item).  Weak: a library built from cem_capi.hip alone (the host sanitizer build) has no lean path and says so
// (cem_planner_rollout_path).
__attribute__((weak)) hipError_t launch_rollout_lean(const RolloutParams &p, int grid, hipStream_t st, bool seg);
// The same launch in the straight-line form (cem_rollout_lean_straight.hip; p.variant picks the objective's instantiation): for the plans
// cem_capi.hip's lean_form gives 2.  Weak for the same reason.
__attribute__((weak)) hipError_t launch_rollout_lean_straight(const RolloutParams &p, int grid, hipStream_t st, bool seg);

// a compile-time int as a value: the exchange-buffer offset of a half-round (cem_rollout_lean_tile.h), a group of the straight-line ring
template <int V> struct LeanConst { static constexpr int value = V; };
