// cem_select_ranked.h — the ranked form of the one-workgroup select (cem_select_ranked.hip): the same SelectParams in,
// the same bits out as cem_select_kernel<true, false> (cem_device.h), in five barrier phases in front of the moments where that kernel
// takes about twelve.  This header is what cem_capi.hip includes: the routing rule and the launcher.  The kernel is compiled in a
// translation unit of its own, as cem_plan_readout.h's is, so that the device code of cem_capi.hip stays what it was.
#pragma once
#include "cem_device.h"

#define CEM_SELECT_RANKED_MAX_N 4096     // a thread of the 1024 owns at most four keys, in registers from the staging to the compaction

// Which form of the one-workgroup select a launch takes: 1, the ranked kernel, where the select resolves to mode 1 with its keys staged
// in LDS (resolve_select_mode: `cache`), the population is at most CEM_SELECT_RANKED_MAX_N and the plain — not the CROWDED —
// instantiation would have been launched (`plain`: the CemMpc objective); else 0, exactly what was launched before this form existed.
inline int select_ranked_form(const int mode, const bool cache, const long long N, const bool plain)
{
    return mode == 1 && cache && N <= CEM_SELECT_RANKED_MAX_N && plain ? 1 : 0;
}

// Weak: a library built without cem_select_ranked.hip launches cem_select_kernel everywhere (form 0).
// prepare: asks the device for `bytes` of dynamic LDS for the kernel (once per handle, as for cem_select_kernel); launch: one workgroup
// of 1024 threads per problem.
__attribute__((weak)) hipError_t prepare_select_ranked(size_t bytes);
__attribute__((weak)) hipError_t launch_select_ranked(const SelectParams &p, int n_problems, size_t lds_bytes, hipStream_t st);
