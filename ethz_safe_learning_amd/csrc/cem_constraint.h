// cem_constraint.h — the cost-minimising objective of SafeCemMpc.optimize_for_safety (safe_cem_mpc.py:40-74): scores = -compute_mean_costs
// (:98-108), the particle mean of the UN-masked cumulative cost.  The cost bytes come from the unchanged rollout kernels (or from
// cem_objective_kernel for the standalone op) run as the safe variant with a goal threshold of -inf: `ga` of CEM_BOOKKEEP is then never
// true, DONE never sets, and the byte a step stores is the plain cost of its state (cem_capi.hip, cem_planner::sc_roll).  What is left
// is this reduction.  Included from cem_capi.hip behind cem_device.h (CtrlBlock).
#pragma once

struct ConstraintReduceParams {
    const uint8_t *costs;        // [H][P][Nloc] un-masked cost of every (step, particle, candidate)
    float *scores;               // [Nloc]  -(sum over steps and particles) / P
    const CtrlBlock *ctrl;
    int32_t Nloc, P, H, check_done;
    uint32_t *zero; int32_t zero_n;        // words block 0 clears for the multi-workgroup select that follows (as ReduceParams::zero), or null
    // batched plans: blockIdx.y is the problem; its costs / scores are the next [H][P][Nloc] / [Nloc] slices, its control block ctrl[blockIdx.y]
};

// One block = 64 candidates (one per lane) x 16 waves, the load shape of cem_reduce_kernel: a latency chain of a few hundred bytes per
// candidate, so what counts is the round trips a wave makes.  The (step, particle) pairs of a candidate are the rows j = t P + p of the
// [H P][Nloc] byte matrix; wave w counts rows w, w + 16, ..., sixteen loads in flight per trip (the shipped P = 45, H = 8: two trips),
// every wave leaves its integer partial in LDS and wave 0 adds the sixteen and stores.  Costs are small integers (at most
// CEM_MAX_COST_KINDS per step): the count is exact, in any order, and equals the reference's fp32 sums; the division by P is the one
// rounding (the reference's reduce_mean: sum / P).
#define CEM_CONSTRAINT_THREADS 1024
#define CEM_CONSTRAINT_TRIP 16
__global__ __launch_bounds__(CEM_CONSTRAINT_THREADS) void cem_constraint_reduce_kernel(const ConstraintReduceParams p)
{
    __shared__ uint32_t cnt_s[16][64];
    const int b = (int)blockIdx.y;
    if (p.check_done && p.ctrl[b].done) return;
    if (p.zero && blockIdx.x == 0 && b == 0) for (int i = threadIdx.x; i < p.zero_n; i += CEM_CONSTRAINT_THREADS) p.zero[i] = 0u;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane;
    const bool live = n < p.Nloc;
    const int nn = live ? n : p.Nloc - 1;
    const int HP = p.H * p.P;                                          // (H P Nloc fits an int32: validate(), cem_compute_objective)
    const uint8_t *const c = p.costs + (size_t)b * HP * p.Nloc + nn;
    uint32_t cnt = 0;
    for (int j0 = w; j0 < HP; j0 += 16 * CEM_CONSTRAINT_TRIP) {
        uint32_t v[CEM_CONSTRAINT_TRIP];
#pragma unroll
        for (int i = 0; i < CEM_CONSTRAINT_TRIP; ++i) { const int j = j0 + 16 * i; v[i] = c[(size_t)(j < HP ? j : j0) * p.Nloc]; }   // (clamped: the loads are unconditional)
#pragma unroll
        for (int i = 0; i < CEM_CONSTRAINT_TRIP; ++i) if (j0 + 16 * i < HP) cnt += v[i];
    }
    cnt_s[w][lane] = cnt;
    __syncthreads();
    if (w != 0 || !live) return;
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) total += cnt_s[i][lane];
    p.scores[(size_t)b * p.Nloc + n] = -((float)total / (float)p.P);   // scores = -mean_costs (safe_cem_mpc.py:61,108)
}
