// cem_constrained.h — budget-constrained planning (cem_mpc.h, cem_planner_set_constraint, CEM_CONSTRAINT_BUDGET): maximise
// the return subject to `predicted cumulative cost <= budget` (constrained CEM, Wen & Topcu 2018).  On a CEM_VARIANT_SAFE handle the
// unchanged rollout kernels (or cem_objective_kernel for the standalone op) leave the done-masked per-particle returns ret[P][Nloc] and
// per-step cost bytes costs[H][P][Nloc]; what is left is this reduction, launched where cem_reduce_kernel would be.  For candidate n:
//   c_p  = sum over t of costs[t][p][n]                                     (an integer)
//   T    = the sum of the m largest c_p                                     (m = P: every particle, the particle mean of the cost;
//                                                                            m < P: its upper tail, CVaR at level m / P)
//   C    = (float)T / (float)m                                              (one division)          -> cstat[n]
//   R    = (((0.f + r_0) + r_1) + ... + r_{P-1}) / (float)P                 (cem_reduce_kernel's particle mean, operation for operation)
//   score = C <= budget ? R : cem_f32_encode_infeasible(T) = -(float)(2^23 + T) * 2^77
// so one ordering holds both rules: feasible candidates by return, below all of them the infeasible ones by ascending cost.  The Beta
// filter and posterior_mean_threashold play no part.  The budget is read from device memory (budget[blockIdx.y]): a captured graph
// follows cem_planner_set_cost_budget.  Included from cem_capi.hip behind cem_device.h (CtrlBlock) and cem_mpc.h (the encoding).
#pragma once
#include "../../include/cem_mpc.h"

struct ConstrainedBudgetParams {
    const float *ret;            // [P][Nloc] per-particle returns of the last rollout
    const uint8_t *costs;        // [H][P][Nloc] masked per-step cost
    float *scores;               // [Nloc]
    float *cstat;                // [Nloc] the cost statistic C
    const float *budget;         // [problems]
    const CtrlBlock *ctrl;
    int32_t Nloc, P, H, m, check_done;     // m in 1 .. P; m == P is the mean form
    uint32_t *zero; int32_t zero_n;        // words block 0 clears for the multi-workgroup select that follows (as ReduceParams::zero), or null
    // batched plans: blockIdx.y is the problem; its ret / costs / scores / cstat are the next [P][Nloc] / [H][P][Nloc] / [Nloc] / [Nloc]
    // slices, its budget budget[blockIdx.y], its control block ctrl[blockIdx.y]
};

#define CEM_BUDGET_THREADS 1024
#define CEM_BUDGET_TRIP 16
#define CEM_BUDGET_MAX_TAIL_P 128
// dynamic LDS, 32-bit words: part_s [16][64]; the tail form adds col_s [P][64]  (P = 45: 15.25 KiB, P = 128: 36 KiB)
#define CEM_BUDGET_LDS_BYTES(P, m) ((size_t)(16 * 64 + ((m) < (P) ? (P) * 64 : 0)) * 4)

// The mean form: the (step, particle) pairs of a candidate are the rows j = t P + p of the [H P][Nloc] byte matrix; wave w counts rows
// w, w + 16, ..., sixteen loads in flight per trip (cem_constraint_reduce_kernel's loop).  Integers: exact in any order.  Offsets within
// a problem's bytes are 32-bit (H P Nloc fits an int32: validate(), cem_compute_objective), and the wave index is a scalar, so a load's
// address is a uniform row pointer plus the lane's candidate: the one vector register every load of the kernel shares.
__device__ __forceinline__ uint32_t cem_budget_count_all(const uint8_t *c, int HP, int Nloc, int w, uint32_t nn)
{
    uint32_t cnt = 0;
    for (int j0 = w; j0 < HP; j0 += 16 * CEM_BUDGET_TRIP) {
        uint32_t v[CEM_BUDGET_TRIP];
#pragma unroll
        for (int i = 0; i < CEM_BUDGET_TRIP; ++i) { const int j = j0 + 16 * i; v[i] = (c + (uint32_t)(j < HP ? j : j0) * (uint32_t)Nloc)[nn]; }   // (clamped: the loads are unconditional)
#pragma unroll
        for (int i = 0; i < CEM_BUDGET_TRIP; ++i) if (j0 + 16 * i < HP) cnt += v[i];
    }
    return cnt;
}

// The tail form: wave w owns particles w, w + 16, ... (J of them at most, in registers).  It sums each over the H steps (16 / J steps,
// hence sixteen loads, per trip), leaves c_p in the LDS column of its lane, and after a barrier ranks each of its particles against all P
// of the column by counting those that come before it in (count descending, index ascending) order — a permutation of 0 .. P-1, so
// exactly m particles have rank < m.  Returns the wave's share of T.  Every LDS access is one dword per lane at bank lane % 32.
template <int J>
__device__ __forceinline__ uint32_t cem_budget_count_tail(const uint8_t *c, int H, int P, int Nloc, int m, int w, int lane, uint32_t nn, uint32_t *col_s)
{
    constexpr int TS = CEM_BUDGET_TRIP / J;                            // steps per trip
    const uint32_t Bloc = (uint32_t)P * (uint32_t)Nloc;
    uint32_t cp[J];
    uint32_t off[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { cp[j] = 0; const int q = w + 16 * j; off[j] = (uint32_t)(q < P ? q : 0) * (uint32_t)Nloc; }   // (clamped: the loads are unconditional, a particle past P is never used)
    for (int t0 = 0; t0 < H; t0 += TS) {
        uint32_t v[TS][J];
#pragma unroll
        for (int s = 0; s < TS; ++s) {
            const uint32_t row = (uint32_t)(t0 + s < H ? t0 + s : t0) * Bloc;
#pragma unroll
            for (int j = 0; j < J; ++j) v[s][j] = (c + (row + off[j]))[nn];
        }
#pragma unroll
        for (int s = 0; s < TS; ++s)
            if (t0 + s < H) {
#pragma unroll
                for (int j = 0; j < J; ++j) cp[j] += v[s][j];
            }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P) col_s[(w + 16 * j) * 64 + lane] = cp[j];
    __syncthreads();
    int rk[J];
#pragma unroll
    for (int j = 0; j < J; ++j) rk[j] = 0;
    for (int q = 0; q < P; ++q) {
        const uint32_t x = col_s[q * 64 + lane];
#pragma unroll
        for (int j = 0; j < J; ++j) rk[j] += (x > cp[j] || (x == cp[j] && q < w + 16 * j)) ? 1 : 0;
    }
    uint32_t part = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P && rk[j] < m) part += cp[j];
    return part;
}

// One block = 64 candidates (one per lane) x 16 waves, the load shape of cem_reduce_kernel and cem_constraint_reduce_kernel: a latency
// chain, so what counts is the round trips a wave makes.  Wave 0's return loads go out first and are in flight while the costs are
// counted; every wave leaves its integer share of T in LDS; wave 0 adds the sixteen, forms C and the score and stores both.
__global__ __launch_bounds__(CEM_BUDGET_THREADS) void cem_constrained_budget_kernel(const ConstrainedBudgetParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cem_budget_lds[];
    uint32_t *const part_s = cem_budget_lds;                           // [16][64]
    uint32_t *const col_s = cem_budget_lds + 16 * 64;                  // [P][64], the tail form only
    const int b = (int)blockIdx.y;
    if (p.check_done && p.ctrl[b].done) return;
    if (p.zero && blockIdx.x == 0 && b == 0) for (int i = threadIdx.x; i < p.zero_n; i += CEM_BUDGET_THREADS) p.zero[i] = 0u;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (the wave index, as a scalar)
    const int n = blockIdx.x * 64 + lane;
    const bool live = n < p.Nloc;
    const uint32_t nn = (uint32_t)(live ? n : p.Nloc - 1);
    const int P = p.P, H = p.H, m = p.m;
    const float *const ret = p.ret + (size_t)b * P * p.Nloc;
    const uint8_t *const c = p.costs + (size_t)b * H * P * p.Nloc;
    // wave 0: the first 16 particles' returns, in flight while the costs are counted
    float r0[16];
    if (w == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) r0[j] = (ret + (size_t)(j < P ? j : 0) * p.Nloc)[nn];
    }
    uint32_t part;
    if (m >= P) part = cem_budget_count_all(c, H * P, p.Nloc, w, nn);
    else {
        const int per_wave = (P + 15) >> 4;                            // particles the busiest wave owns (uniform)
        if (per_wave <= 1) part = cem_budget_count_tail<1>(c, H, P, p.Nloc, m, w, lane, nn, col_s);
        else if (per_wave <= 2) part = cem_budget_count_tail<2>(c, H, P, p.Nloc, m, w, lane, nn, col_s);
        else if (per_wave <= 4) part = cem_budget_count_tail<4>(c, H, P, p.Nloc, m, w, lane, nn, col_s);
        else part = cem_budget_count_tail<8>(c, H, P, p.Nloc, m, w, lane, nn, col_s);
    }
    part_s[w * 64 + lane] = part;
    float sum = 0.f;
    if (w == 0) {                                                      // cem_reduce_kernel's sum: q = 0 .. P-1 in that order
#pragma unroll
        for (int j = 0; j < 16; ++j) if (j < P) sum = sum + r0[j];
        for (int q = 16; q < P; q += 16) {
            float v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = (ret + (size_t)(q + j < P ? q + j : q) * p.Nloc)[nn];
#pragma unroll
            for (int j = 0; j < 16; ++j) if (q + j < P) sum = sum + v[j];
        }
    }
    __syncthreads();
    if (w != 0 || !live) return;
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) total += part_s[i * 64 + lane];
    const float cst = (float)total / (float)m;
    const float budget = p.budget[b];
    p.cstat[(size_t)b * p.Nloc + n] = cst;
    p.scores[(size_t)b * p.Nloc + n] = cst <= budget ? sum / (float)P : cem_f32_encode_infeasible((int32_t)total);
}

// the launch: grid.x = blocks of 64 candidates, grid.y = problems of a batched plan
static inline hipError_t launch_constrained_budget(const ConstrainedBudgetParams &p, int n_problems, hipStream_t stream)
{
    hipLaunchKernelGGL(cem_constrained_budget_kernel, dim3((p.Nloc + 63) / 64, n_problems), dim3(CEM_BUDGET_THREADS), CEM_BUDGET_LDS_BYTES(p.P, p.m), stream, p);
    return hipGetLastError();
}
