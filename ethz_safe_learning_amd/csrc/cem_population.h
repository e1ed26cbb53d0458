// cem_population.h — per-iteration population sizes and the mean candidate (cem_planner_set_population_schedule,
// cem_planner_set_mean_candidate).
//
// The schedule needs no kernel: iteration `it` of a scheduled plan is launched as a handle of n_samples = n[it] would launch it — its own
// Dims, tile list, segments, sampler placement and select form, all from the functions create uses (cem_capi.hip) — on the arrays the
// handle already has, of which it fills the leading n[it] entries.
//
// The mean candidate is one kernel between the sampler launch (cem_sample_kernel) and the rollout launch of the LAST iteration, behind the
// elite inject where that runs: row `row` (the iteration's last candidate) of both action layouts becomes
//     min(max(mu[t][a], lb[a]), ub[a])
// from the mu the iteration samples from.  The sampler has drawn that row like any other (no Philox counter moves); the padding words of
// act_pad keep their zeros.  planner.mean_candidate restates it in NumPy.  One thread per (step, action quad), grid.y the problem; a
// problem that is `done` is left alone.  No LDS, no atomics; the only floating-point work is the min and the max.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_population.hip defines
// CEM_POPULATION_UNIT), as cem_elite_carry.h's are, so that the device code of the other units stays what it was.
#pragma once
#include "cem_device.h"

#define CEM_MEAN_THREADS 256

struct MeanCandidateParams {
    const float *musig;          // [problems][2][H][A]: mu, then sigma (only mu is read)
    const float *act_bounds;     // lb at [a], ub at [32 + a]
    const CtrlBlock *ctrl;       // [problems]
    float *actions;              // [problems][N][H][A]
    float *act_pad;              // [problems][N][H][pad_floats]: action a of (n, t) at word pad_shift + a
    int32_t N, row, H, A, pad_shift, pad_floats;
};

// Weak: a library built without cem_population.hip has no mean candidate and cem_planner_set_mean_candidate says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_mean_candidate(const MeanCandidateParams &p, int n_problems, hipStream_t st);

#ifdef CEM_POPULATION_UNIT
__global__ __launch_bounds__(CEM_MEAN_THREADS) void cem_mean_candidate_kernel(const MeanCandidateParams p)
{
    const int b = (int)blockIdx.y;
    if (p.ctrl[b].done) return;
    const int H = p.H, A = p.A, AZ = (A + 3) >> 2;
    const int q = (int)(blockIdx.x * CEM_MEAN_THREADS + threadIdx.x);
    if (q >= H * AZ) return;
    const int z = q % AZ, t = q / AZ;
    const float *mu = p.musig + (size_t)b * 2 * H * A + (size_t)t * A;
    float *nat = p.actions + (((size_t)b * p.N + p.row) * H + t) * A;
    float *pad = p.act_pad + (((size_t)b * p.N + p.row) * H + t) * p.pad_floats + p.pad_shift;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int a = 4 * z + r;
        if (a < A) { const float v = fminf(fmaxf(mu[a], p.act_bounds[a]), p.act_bounds[32 + a]); nat[a] = v; pad[a] = v; }
    }
}

hipError_t launch_mean_candidate(const MeanCandidateParams &p, int n_problems, hipStream_t st)
{
    const int total = p.H * ((p.A + 3) / 4);
    hipLaunchKernelGGL(cem_mean_candidate_kernel, dim3((total + CEM_MEAN_THREADS - 1) / CEM_MEAN_THREADS, n_problems), dim3(CEM_MEAN_THREADS), 0, st, p);
    return hipGetLastError();
}
#endif
