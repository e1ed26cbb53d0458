// cem_score.h — the score stage: how the P particles of a candidate become its score.  The rollout kernels (or cem_objective_kernel for
// the standalone op) leave the per-particle returns ret[P][Nloc] and, on the safe variant, the per-step cost bytes costs[H][P][Nloc];
// one of four kernels, chosen by the handle's objective (cem_capi.hip, launch_score), reduces them:
//   cem_reduce_kernel              mpc_policy.py:38-39, safe_cem_mpc.py:94-96,110-120   particle mean, Beta safety filter
//   cem_constraint_reduce_kernel   safe_cem_mpc.py:40-74,98-108 (CEM_VARIANT_COST)        -(particle mean of the un-masked cumulative cost)
//   cem_constraint_tail_kernel     cem_planner_set_particle_objective, LOWER_TAIL         mean of the m smallest returns, Beta safety filter
//   cem_constrained_budget_kernel  cem_planner_set_constraint, BUDGET     particle mean within a cost budget
// All four are one block = 64 candidates (one per lane) x 16 waves: a latency chain of a few hundred bytes per candidate, one dependent
// round of loads, a barrier, a store — so what matters is how many round trips to L2 a wave makes, not bandwidth.  They are compositions
// of the pieces below, each defined once: what two objectives share (the Beta counts, the ordered particle mean, the byte-row count, the
// ranking within a candidate's LDS column) is the same code, hence the same arithmetic in the same order.
// Included from cem_capi.hip behind cem_device.h (CtrlBlock).
#pragma once
#include "../../include/cem_mpc.h"
#include <type_traits>

struct ReduceParams {
    const float *ret; const uint8_t *costs; float *scores; const CtrlBlock *ctrl;
    int32_t Nloc, P, H, variant, check_done;
    float alpha, beta, thr;
    uint32_t *zero; int32_t zero_n;        // words block 0 clears for the multi-workgroup select that follows (digit histograms + barrier counter), or null
    int32_t m;                             // the tail kernel: the m smallest returns; the budget kernel: the m largest costs (m == P: the mean form)
    float *cstat;                          // the budget kernel: [Nloc] the cost statistic C
    const float *budget;                   // the budget kernel: [problems]
    // batched plans: blockIdx.y is the problem; its ret / costs / scores / cstat are the next [P][Nloc] / [H][P][Nloc] / [Nloc] / [Nloc]
    // slices, its budget budget[blockIdx.y], its control block ctrl[blockIdx.y]
};

#define CEM_SCORE_THREADS 1024
#define CEM_SCORE_TRIP 16                  // loads a wave keeps in flight per round trip
#define CEM_TAIL_MAX_P 128                 // the ranking kernels hold eight particles per wave in registers and P x 64 values in LDS
#define CEM_BUDGET_MAX_TAIL_P CEM_TAIL_MAX_P
// dynamic LDS of the tail kernel, 32-bit words: unsafe_w [16][64], cnt_s [16][64], ret_s [P][64]  (P = 45: 19.25 KiB, P = 128: 40 KiB)
#define CEM_TAIL_LDS_BYTES(P) ((size_t)(2 * 16 * 64 + (P) * 64) * 4)
// dynamic LDS of the budget kernel: part_s [16][64]; the tail form adds col_s [P][64]  (P = 45: 15.25 KiB, P = 128: 36 KiB)
#define CEM_BUDGET_LDS_BYTES(P, m) ((size_t)(16 * 64 + ((m) < (P) ? (P) * 64 : 0)) * 4)

// where a thread stands: problem b, wave w, candidate n of lane `lane`; nn is n clamped into the problem (the loads are unconditional)
struct ScoreLane { int b, lane, w, n, nn; bool live; };

// The prologue of every score kernel, in two statements: `if (cem_score_done(p)) return;` — a finished plan's block leaves at once (the
// return stands in the kernel itself: behind an inlined call the same test costs cem_reduce_kernel vector registers) — and
// cem_score_prologue: block 0 clears the select's words, every thread finds where it stands.  SCALAR_W: the wave index is read with
// readfirstlane, so what is computed from it (row offsets, the `wave 0` branches) is scalar: vector registers saved in the kernels that
// count byte rows, scalar registers the two that run the Beta counts cannot spare.
__device__ __forceinline__ bool cem_score_done(const ReduceParams &p) { return p.check_done && p.ctrl[(int)blockIdx.y].done; }

template <bool SCALAR_W>
__device__ __forceinline__ ScoreLane cem_score_prologue(const ReduceParams &p)
{
    ScoreLane s;
    s.b = (int)blockIdx.y;
    if (p.zero && blockIdx.x == 0 && s.b == 0) for (int i = threadIdx.x; i < p.zero_n; i += CEM_SCORE_THREADS) p.zero[i] = 0u;
    s.lane = threadIdx.x & 63; s.w = SCALAR_W ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
    s.n = blockIdx.x * 64 + s.lane;
    s.live = s.n < p.Nloc;
    s.nn = s.live ? s.n : p.Nloc - 1;
    return s;
}

// The per-step Beta counts (safe_cem_mpc.py:90-96,110-120): the OR over this wave's steps of (alpha + count_t) / ((alpha + beta) + P) > thr.
//   * horizons of 16 steps and more: wave w counts the particle costs of steps t = w, w + 16, ..., TWO steps per trip, up to 8 particles each;
//   * shorter horizons: the 16 waves share out (step, particle slice) pairs — 16 / H waves per step, each counting every (16 / H)-th
//     particle, up to 16 loads per trip — and add their counts in cnt_s [16][64].
// Counts are small integers: exact, order-free, and exact in the reference's fp32 sums as well.  Every wave of the block calls it (it
// holds barriers).
__device__ __forceinline__ int32_t cem_beta_unsafe(const ReduceParams &p, const uint8_t *costs, int nn, int w, int lane, uint32_t (*cnt_s)[64])
{
    const int P = p.P, H = p.H;
    const float denom = (p.alpha + p.beta) + (float)P;
    const size_t Bloc = (size_t)P * p.Nloc;
    int32_t unsafe = 0;
    if (H >= 16) {
        for (int t = w; t < H; t += 32) {
            const int t2 = t + 16 < H ? t + 16 : t;                   // (clamped: the loads are unconditional, the second count is dropped)
            const uint8_t *ca = costs + (size_t)t * Bloc + nn, *cb = costs + (size_t)t2 * Bloc + nn;
            uint32_t cnta = 0, cntb = 0;
            for (int q = 0; q < P; q += 8) {
                uint32_t va[8], vb[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) { const size_t o = (size_t)(q + j < P ? q + j : q) * p.Nloc; va[j] = ca[o]; vb[j] = cb[o]; }
#pragma unroll
                for (int j = 0; j < 8; ++j) if (q + j < P) { cnta += va[j]; cntb += vb[j]; }
            }
            unsafe |= ((p.alpha + (float)cnta) / denom <= p.thr) ? 0 : 1;
            if (t + 16 < H) unsafe |= ((p.alpha + (float)cntb) / denom <= p.thr) ? 0 : 1;
        }
    } else {
        const int wpt = 16 / H;                                        // waves per step (>= 1), H * wpt <= 16 of the waves count
        cnt_s[w][lane] = 0u;
        __syncthreads();
        if (w < H * wpt) {
            const int t = w / wpt, part = w % wpt;
            const uint8_t *c = costs + (size_t)t * Bloc + nn;
            uint32_t cnt = 0;
            for (int q = part; q < P; q += 16 * wpt) {
                uint32_t v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) { const int qq = q + j * wpt; v[j] = c[(size_t)(qq < P ? qq : q) * p.Nloc]; }
#pragma unroll
                for (int j = 0; j < 16; ++j) if (q + j * wpt < P) cnt += v[j];
            }
            if (wpt > 1) atomicAdd(&cnt_s[t][lane], cnt); else cnt_s[t][lane] = cnt;
        }
        __syncthreads();
        if (w < H) unsafe = ((p.alpha + (float)cnt_s[w][lane]) / denom <= p.thr) ? 0 : 1;
    }
    return unsafe;
}

// wave 0, behind the block's barrier: a candidate with an unsafe step in any wave's unsafe_w [16][64] loses 100 (safe_cem_mpc.py:94-96)
__device__ __forceinline__ float cem_beta_filter(float score, const int32_t (*unsafe_w)[64], int lane)
{
    int32_t u = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) u |= unsafe_w[i][lane];
    return score - (u ? 1.0f : 0.0f) * 100.0f;
}

// The particle mean (mpc_policy.py:38-39) of wave 0, in two halves: the first 16 particles' returns are requested before the wave's
// cost loads and stay in flight while the costs are counted (I: the type of the lane's candidate offset, the caller's own) ...
struct MeanHead { float r[16]; };
template <typename I>
__device__ __forceinline__ MeanHead cem_mean_issue(const float *ret, int P, int Nloc, I nn)
{
    MeanHead h;
#pragma unroll
    for (int j = 0; j < 16; ++j) h.r[j] = (ret + (size_t)(j < P ? j : 0) * Nloc)[nn];
    return h;
}

// ... and the sum in the reference's order, (((0.f + r_0) + r_1) + ... + r_{P-1}), 16 loads per further trip.  The caller divides it by
// (float)P, once, behind the barrier (reduce_mean over particles).  The first sixteen travel between the halves as a value (MeanHead): as
// an array handed in by reference, the waves that load nothing set sixteen registers to zero in cem_reduce_kernel.
template <typename I>
__device__ __forceinline__ float cem_mean_finish(const float *ret, int P, int Nloc, I nn, const MeanHead &h)
{
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < P) sum = sum + h.r[j];
    for (int q = 16; q < P; q += 16) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) v[j] = (ret + (size_t)(q + j < P ? q + j : q) * Nloc)[nn];
#pragma unroll
        for (int j = 0; j < 16; ++j) if (q + j < P) sum = sum + v[j];
    }
    return sum;
}

// The byte-row count: the (step, particle) pairs of a candidate are the rows j = t P + p of the [H P][Nloc] byte matrix; wave w counts
// rows w, w + 16, ..., sixteen loads in flight per trip (the shipped P = 45, H = 8: two trips).  Integers: exact in any order.  Offsets
// within a problem's bytes are 32-bit (H P Nloc fits an int32: validate(), cem_compute_objective), and the wave index is a scalar, so a
// load's address is a uniform row pointer plus the lane's candidate: the one vector register every load shares.
__device__ __forceinline__ uint32_t cem_count_rows(const uint8_t *c, int HP, int Nloc, int w, uint32_t nn)
{
    uint32_t cnt = 0;
    for (int j0 = w; j0 < HP; j0 += 16 * CEM_SCORE_TRIP) {
        uint32_t v[CEM_SCORE_TRIP];
#pragma unroll
        for (int i = 0; i < CEM_SCORE_TRIP; ++i) { const int j = j0 + 16 * i; v[i] = (c + (uint32_t)(j < HP ? j : j0) * (uint32_t)Nloc)[nn]; }   // (clamped: the loads are unconditional)
#pragma unroll
        for (int i = 0; i < CEM_SCORE_TRIP; ++i) if (j0 + 16 * i < HP) cnt += v[i];
    }
    return cnt;
}

// wave 0, behind the block's barrier: the sum of the sixteen waves' integer partials part_s [16][64]
__device__ __forceinline__ uint32_t cem_sum_partials(const uint32_t *part_s, int lane)
{
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) total += part_s[i * 64 + lane];
    return total;
}

// The ranking within a candidate's LDS column [P][64]: wave w owns particles w, w + 16, ... (J of them at most, in registers) and counts
// for each, over the column's rows q = 0 .. P-1, those that come before it in (value, particle index) order — a permutation of 0 .. P-1,
// so exactly m particles have rank < m.  This is that order, ascending or DESCending by value with ties in index order: whether row q
// (value x) comes before the held particle idx (value v).  It takes scalars only: handed the register arrays, the same loop compiles to
// selects instead of branches and costs the tail kernel vector and scalar registers it had not used before.  Every LDS access of the loops that
// call it is one dword per lane at bank lane % 32: no conflicts.  The two loops (cem_tail_body, cem_budget_count_tail) are the same five
// lines but for the element type and DESC, and must stay so: a change to one is a change to both.
template <bool DESC, typename T>
__device__ __forceinline__ int cem_comes_before(T x, int q, T v, int idx) { return ((DESC ? x > v : x < v) || (x == v && q < idx)) ? 1 : 0; }

// f(integral_constant<int, J>) for the smallest J of 1, 2, 4, 8 that holds the particles the busiest wave owns (uniform; P <= CEM_TAIL_MAX_P)
template <typename F>
__device__ __forceinline__ void cem_dispatch_j(int P, F &&f)
{
    const int per_wave = (P + 15) >> 4;
    if (per_wave <= 1) f(std::integral_constant<int, 1>{});
    else if (per_wave <= 2) f(std::integral_constant<int, 2>{});
    else if (per_wave <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

// ---------------------------------------------------------------------------------------------------------
// the particle mean and the Beta filter.  Wave 0's return loads are requested before its cost loads.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CEM_SCORE_THREADS) void cem_reduce_kernel(const ReduceParams p)
{
    __shared__ int32_t unsafe_w[16][64];
    __shared__ uint32_t cnt_s[16][64];
    if (cem_score_done(p)) return;
    const ScoreLane s = cem_score_prologue<false>(p);
    const float *const ret = p.ret + (size_t)s.b * p.P * p.Nloc;
    const uint8_t *const costs = p.costs ? p.costs + (size_t)s.b * p.H * p.P * p.Nloc : p.costs;
    MeanHead r0;
    if (s.w == 0) r0 = cem_mean_issue(ret, p.P, p.Nloc, s.nn);
    if (p.variant == 1) unsafe_w[s.w][s.lane] = cem_beta_unsafe(p, costs, s.nn, s.w, s.lane, cnt_s);
    float score = 0.f;
    if (s.w == 0) score = cem_mean_finish(ret, p.P, p.Nloc, s.nn, r0);
    __syncthreads();
    if (s.w != 0 || !s.live) return;
    score = score / (float)p.P;                                        // reduce_mean over particles
    if (p.variant == 1) score = cem_beta_filter(score, unsafe_w, s.lane);
    p.scores[(size_t)s.b * p.Nloc + s.n] = score;
}

// ---------------------------------------------------------------------------------------------------------
// the cost-minimising objective of SafeCemMpc.optimize_for_safety (safe_cem_mpc.py:40-74): scores = -compute_mean_costs (:98-108), the
// particle mean of the UN-masked cumulative cost.  The cost bytes come from the safe variant run with a goal threshold of -inf: `ga` of
// CEM_BOOKKEEP is then never true, DONE never sets, and the byte a step stores is the plain cost of its state (cem_capi.hip,
// cem_planner::sc_roll).  Every wave leaves its integer partial in LDS, wave 0 adds the sixteen; costs are small integers (at most
// CEM_MAX_COST_KINDS per step), so the count equals the reference's fp32 sums and the division by P is the one rounding (sum / P).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CEM_SCORE_THREADS) void cem_constraint_reduce_kernel(const ReduceParams p)
{
    __shared__ uint32_t cnt_s[16][64];
    if (cem_score_done(p)) return;
    const ScoreLane s = cem_score_prologue<true>(p);
    const int HP = p.H * p.P;
    cnt_s[s.w][s.lane] = cem_count_rows(p.costs + (size_t)s.b * HP * p.Nloc, HP, p.Nloc, s.w, (uint32_t)s.nn);
    __syncthreads();
    if (s.w != 0 || !s.live) return;
    p.scores[(size_t)s.b * p.Nloc + s.n] = -((float)cem_sum_partials(&cnt_s[0][0], s.lane) / (float)p.P);   // scores = -mean_costs (safe_cem_mpc.py:61,108)
}

// ---------------------------------------------------------------------------------------------------------
// the risk-averse particle objective (cem_mpc.h, cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL): the mean of the m
// SMALLEST of a candidate's P particle returns (CVaR at level m / P; m = 1: the worst particle) instead of the mean over all of them.
//   value[n] = (((0.f + r_(0)) + r_(1)) + ... + r_(m-1)) / (float)m,  r_(i) the particle returns of candidate n in ascending order of
//   (return, particle index): equal returns go in particle order, -0.f == 0.f.  NaN returns are outside the contract.
// On a CEM_VARIANT_SAFE handle the Beta filter IS cem_reduce_kernel's (cem_beta_unsafe, cem_beta_filter), applied to this value.
// Wave w loads its particles (coalesced over the lanes), leaves them in the LDS column of its lane, and after a barrier ranks them; after
// a second barrier those of rank < m go to row `rank` of the same column and no two writes meet.  Wave 0 then adds rows 0 .. m-1 in
// order, divides, applies the Beta filter and stores.
// ---------------------------------------------------------------------------------------------------------
template <int J>
__device__ __forceinline__ void cem_tail_body(const ReduceParams &p, const ScoreLane &s, const float *ret, const uint8_t *costs, uint32_t *lds)
{
    int32_t *const unsafe_w = (int32_t *)lds;
    uint32_t *const cnt_s = lds + 16 * 64;
    float *const ret_s = (float *)(lds + 2 * 16 * 64);
    const int lane = s.lane, w = s.w, nn = s.nn, P = p.P, m = p.m;
    float v[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { const int q = w + 16 * j; v[j] = ret[(size_t)(q < P ? q : 0) * p.Nloc + nn]; }   // (clamped: the loads are unconditional)
    if (p.variant == 1) unsafe_w[w * 64 + lane] = cem_beta_unsafe(p, costs, nn, w, lane, (uint32_t (*)[64])cnt_s);
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P) ret_s[(w + 16 * j) * 64 + lane] = v[j];
    __syncthreads();
    int rk[J];
#pragma unroll
    for (int j = 0; j < J; ++j) rk[j] = 0;
    for (int q = 0; q < P; ++q) {
        const float x = ret_s[q * 64 + lane];
#pragma unroll
        for (int j = 0; j < J; ++j) rk[j] += cem_comes_before<false>(x, q, v[j], w + 16 * j);   // (the loop of cem_budget_count_tail, ascending)
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P && rk[j] < m) ret_s[rk[j] * 64 + lane] = v[j];
    __syncthreads();
    if (w != 0 || !s.live) return;
    float sum = 0.f;
    for (int i = 0; i < m; ++i) sum = sum + ret_s[i * 64 + lane];
    float score = sum / (float)m;
    if (p.variant == 1) score = cem_beta_filter(score, (const int32_t (*)[64])unsafe_w, lane);
    p.scores[(size_t)s.b * p.Nloc + s.n] = score;
}

__global__ __launch_bounds__(CEM_SCORE_THREADS) void cem_constraint_tail_kernel(const ReduceParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cem_tail_lds[];
    if (cem_score_done(p)) return;
    const ScoreLane s = cem_score_prologue<false>(p);
    const float *const ret = p.ret + (size_t)s.b * p.P * p.Nloc;
    const uint8_t *const costs = p.costs ? p.costs + (size_t)s.b * p.H * p.P * p.Nloc : p.costs;
    cem_dispatch_j(p.P, [&](auto J) __attribute__((always_inline)) { cem_tail_body<decltype(J)::value>(p, s, ret, costs, cem_tail_lds); });
}

// ---------------------------------------------------------------------------------------------------------
// budget-constrained planning (cem_mpc.h, cem_planner_set_constraint, CEM_CONSTRAINT_BUDGET): maximise the return subject
// to `predicted cumulative cost <= budget` (constrained CEM, Wen & Topcu 2018), on a CEM_VARIANT_SAFE handle.  For candidate n:
//   c_p  = sum over t of costs[t][p][n]                                     (an integer)
//   T    = the sum of the m largest c_p                                     (m = P: every particle, the particle mean of the cost;
//                                                                            m < P: its upper tail, CVaR at level m / P)
//   C    = (float)T / (float)m                                              (one division)          -> cstat[n]
//   R    = the particle mean of the returns                                 (cem_mean_issue, cem_mean_finish: cem_reduce_kernel's)
//   score = C <= budget ? R : cem_f32_encode_infeasible(T) = -(float)(2^23 + T) * 2^77
// so one ordering holds both rules: feasible candidates by return, below all of them the infeasible ones by ascending cost.  The Beta
// filter and posterior_mean_threashold play no part.  The budget is read from device memory (budget[blockIdx.y]): a captured graph
// follows cem_planner_set_cost_budget.
// ---------------------------------------------------------------------------------------------------------

// The tail form's share of T for this wave: it sums each of its particles over the H steps (16 / J steps, hence sixteen loads, per trip),
// leaves c_p in the LDS column of its lane, and after a barrier ranks them by (count descending, index ascending).
template <int J>
__device__ __forceinline__ uint32_t cem_budget_count_tail(const uint8_t *c, int H, int P, int Nloc, int m, int w, int lane, uint32_t nn, uint32_t *col_s)
{
    constexpr int TS = CEM_SCORE_TRIP / J;                             // steps per trip
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
        for (int j = 0; j < J; ++j) rk[j] += cem_comes_before<true>(x, q, cp[j], w + 16 * j);   // (the loop of cem_tail_body, descending)
    }
    uint32_t part = 0;
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P && rk[j] < m) part += cp[j];
    return part;
}

// Wave 0's return loads go out first and are in flight while the costs are counted; every wave leaves its integer share of T in LDS;
// wave 0 adds the sixteen, forms C and the score and stores both.
__global__ __launch_bounds__(CEM_SCORE_THREADS) void cem_constrained_budget_kernel(const ReduceParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cem_budget_lds[];
    uint32_t *const part_s = cem_budget_lds;                           // [16][64]
    uint32_t *const col_s = cem_budget_lds + 16 * 64;                  // [P][64], the tail form only
    if (cem_score_done(p)) return;
    const ScoreLane s = cem_score_prologue<true>(p);
    const int lane = s.lane, w = s.w, P = p.P, H = p.H, m = p.m;
    const uint32_t nn = (uint32_t)s.nn;
    const float *const ret = p.ret + (size_t)s.b * P * p.Nloc;
    const uint8_t *const c = p.costs + (size_t)s.b * H * P * p.Nloc;
    MeanHead r0;
    if (w == 0) r0 = cem_mean_issue(ret, P, p.Nloc, nn);
    uint32_t part;
    if (m >= P) part = cem_count_rows(c, H * P, p.Nloc, w, nn);
    else cem_dispatch_j(P, [&](auto J) __attribute__((always_inline)) { part = cem_budget_count_tail<decltype(J)::value>(c, H, P, p.Nloc, m, w, lane, nn, col_s); });
    part_s[w * 64 + lane] = part;
    float mean = 0.f;
    if (w == 0) mean = cem_mean_finish(ret, P, p.Nloc, nn, r0);
    __syncthreads();
    if (w != 0 || !s.live) return;
    const uint32_t total = cem_sum_partials(part_s, lane);
    const float cst = (float)total / (float)m;
    const float budget = p.budget[s.b];
    p.cstat[(size_t)s.b * p.Nloc + s.n] = cst;
    p.scores[(size_t)s.b * p.Nloc + s.n] = cst <= budget ? mean / (float)P : cem_f32_encode_infeasible((int32_t)total);
}
