// cem_refit_weighted.h — the score-weighted refit (cem_mpc.h, cem_planner_set_refit, CEM_REFIT_SOFTMAX): the MPPI /
// "weighted elites" update in place of CEM's uniform one.  The unchanged one-workgroup select runs first, its blend pointed at a scratch
// slice and its early stop and result hand-over switched off by its parameters; it leaves elite_idx[k] (ascending candidate index, ties to
// the lowest), best-so-far and ctrl->iters.  This kernel, one workgroup per problem directly behind it, refits from the scores themselves:
//   s_j    = scores[elite[j]],  s_max = max_j s_j                                  (NaN among the elites: outside the contract)
//   w_j    = s_j == s_max ? 1 : expf((s_j - s_max) * beta)                         beta = fl32(1 / temperature), rounded once on the host
//   W      = sum_j w_j (>= 1),  Q = sum_j w_j^2,  ESS = W * W / Q                  -> stat[problem][iters - 1]
//   mean_c = (sum_j w_j * a_j[c]) / W
//   var_c  = (sum_j w_j * ((a_j[c] - mean_c) * (a_j[c] - mean_c))) / W             two-pass, as tf.nn.moments
//   mu_c   = s * mu_c + fl32(1 - s) * mean_c,  sigma_c = s * sigma_c + fl32(1 - s) * sqrtf(var_c)      (cem_mpc.py:64-65, op for op)
//   stop iff (((0.f + sigma_0) + sigma_1) + ...) / (float)HA <= threshold          (cem_mpc.py:66-67, the select's order) -> ctrl->done
// Summation order (fixed; -ffp-contract=off: no fused multiply-adds; no floating-point atomics — equal inputs give equal bits):
//   W, Q    thread t adds its elites j = t, t + 1024, ... in ascending order from 0.f; the 64 lanes of a wave combine by the xor butterfly
//           (distance 32, 16, ..., 1: x + partner(x), commutative, so every lane holds the same bits); the sixteen wave totals are added
//           in wave order from 0.f.
//   columns a block of ncol = min(HA - cb, 1024) columns is served by tpc = the largest power of two with tpc * ncol <= 1024 parts; part q
//           adds its elites j = q, q + tpc, ... in ascending order from 0.f; the parts are added in part order from 0.f; one division by W.
// Gathers: a thread keeps the first CEM_REFIT_KEEP rows of its part in registers across the two phases; rows beyond them are gathered
// again in each phase, CEM_REFIT_BATCH loads in flight.  The elite indices are read from global memory (the select has just written
// them); the weights live in LDS, one dword per lane at consecutive or equal (broadcast) addresses, as do the partial sums.
// Included from cem_capi.hip behind cem_device.h (CtrlBlock).  The few lines it has in common with cem_select_kernel's moments are copied,
// not shared: that kernel's instruction stream stays what it was.
#pragma once

struct RefitWeightedParams {
    const float *scores;         // [problems][N] the scores the select ranked
    const float *actions;        // [problems][N][HA]
    float *musig;                // [problems][2][HA] the plan's mu / sigma (the select's blend went to a scratch slice)
    CtrlBlock *ctrl;             // [problems]
    const int32_t *elite_idx;    // [problems][k] as the select stored them
    float *stat;                 // [problems][I] effective sample size per iteration
    int32_t N, k, HA, I;
    float beta, smoothing, one_minus_smoothing, threshold;
};

#define CEM_REFIT_THREADS 1024
#define CEM_REFIT_KEEP 4         // rows of a part gathered once and kept in registers for both phases
#define CEM_REFIT_BATCH 4        // gathers in flight per thread beyond them
// dynamic LDS: w[k rounded up to 4] + colmean[HA] + newsig[HA]   (never more than the select's own dynamic LDS for the same shape)
#define CEM_REFIT_LDS_BYTES(k, HA) (((size_t)(((k) + 3) & ~3) + (size_t)2 * (HA)) * 4)

__global__ __launch_bounds__(CEM_REFIT_THREADS) void cem_constraint_refit_kernel(const RefitWeightedParams p)
{
    extern __shared__ __attribute__((aligned(16))) float cem_refit_lds[];
    __shared__ float red[CEM_REFIT_THREADS];      // per-thread partial sums of a column block
    __shared__ float wred[3][16];                 // per-wave max / sum w / sum w^2
    const int prob = (int)blockIdx.x;
    CtrlBlock *const ctrl = p.ctrl + prob;
    if (ctrl->done) return;                       // stopped earlier (or a row of a batch handle that sits this plan out): the select left at once too
    const int tid = threadIdx.x, k = p.k, HA = p.HA;
    const float *const scores_b = p.scores + (size_t)prob * p.N;
    const float *const actions_b = p.actions + (size_t)prob * p.N * HA;
    float *const musig_b = p.musig + (size_t)prob * 2 * HA;
    const int32_t *const elite_b = p.elite_idx + (size_t)prob * k;
    float *const w = cem_refit_lds;                                   // [k] scores, then weights
    float *const colmean = w + ((k + 3) & ~3);                        // [HA]
    float *const newsig = colmean + HA;                               // [HA] smoothed sigma
    // (an elite index is a candidate index by the select's contract; held to the population all the same: no gather leaves the tensor)
    auto elite = [&](const int e) { const int i = elite_b[e]; return (uint32_t)i < (uint32_t)p.N ? i : 0; };

    // ---- the elites' scores and their maximum (exact in any order; -0.0 == +0.0, either may stand for both) ----
    float smax = -__builtin_inff();
    for (int j = tid; j < k; j += CEM_REFIT_THREADS) { const float s = scores_b[elite(j)]; w[j] = s; smax = s > smax ? s : smax; }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { const float o = __shfl_xor(smax, d); smax = o > smax ? o : smax; }
    if ((tid & 63) == 0) wred[0][tid >> 6] = smax;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) { const float o = wred[0][i]; smax = o > smax ? o : smax; }

    // ---- weights, W and Q ----
    float sw = 0.f, sq = 0.f;
    for (int j = tid; j < k; j += CEM_REFIT_THREADS) {                // (a thread's own words: no barrier between the two loops)
        const float s = w[j];
        const float wj = s == smax ? 1.f : expf((s - smax) * p.beta);
        w[j] = wj; sw = sw + wj; sq = sq + wj * wj;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { sw = sw + __shfl_xor(sw, d); sq = sq + __shfl_xor(sq, d); }
    if ((tid & 63) == 0) { wred[1][tid >> 6] = sw; wred[2][tid >> 6] = sq; }
    __syncthreads();                                                  // (w[] is complete for every thread from here on)
    float W = 0.f, Q = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { W = W + wred[1][i]; Q = Q + wred[2][i]; }

    // ---- weighted moments, column block by column block ----
    const float sm = p.smoothing, osm = p.one_minus_smoothing;
    for (int cb = 0; cb < HA; cb += CEM_REFIT_THREADS) {
        const int ncol = (HA - cb < CEM_REFIT_THREADS) ? HA - cb : CEM_REFIT_THREADS;
        int tpc = 1; while (tpc * 2 * ncol <= CEM_REFIT_THREADS) tpc *= 2;
        const int part = tid / ncol, col = tid % ncol;
        const bool act = part < tpc;
        // old mu / sigma of the column this thread finishes: requested now, needed at the end of the block
        float old_mu = 0.f, old_sg = 0.f;
        if (part == 0) { old_mu = musig_b[cb + col]; old_sg = musig_b[HA + cb + col]; }
        float av[CEM_REFIT_KEEP], wv[CEM_REFIT_KEEP];
#pragma unroll
        for (int j = 0; j < CEM_REFIT_KEEP; ++j) {
            const int e = part + j * tpc;
            const bool ok = act && e < k;
            wv[j] = ok ? w[e] : 0.f;
            av[j] = ok ? actions_b[(size_t)elite(e) * HA + cb + col] : 0.f;
        }
        for (int phase = 0; phase < 2; ++phase) {
            float acc = 0.f;
            const float m = phase ? colmean[cb + col] : 0.f;
            if (act) {
#pragma unroll
                for (int j = 0; j < CEM_REFIT_KEEP; ++j)
                    if (part + j * tpc < k) { const float a = av[j]; acc = phase ? acc + wv[j] * ((a - m) * (a - m)) : acc + wv[j] * a; }
                for (int e0 = part + CEM_REFIT_KEEP * tpc; e0 < k; e0 += CEM_REFIT_BATCH * tpc) {     // same summation order
                    float b[CEM_REFIT_BATCH], wb[CEM_REFIT_BATCH];
#pragma unroll
                    for (int j = 0; j < CEM_REFIT_BATCH; ++j) {
                        const int e = e0 + j * tpc;
                        wb[j] = e < k ? w[e] : 0.f;
                        b[j] = e < k ? actions_b[(size_t)elite(e) * HA + cb + col] : 0.f;
                    }
#pragma unroll
                    for (int j = 0; j < CEM_REFIT_BATCH; ++j)
                        if (e0 + j * tpc < k) { const float a = b[j]; acc = phase ? acc + wb[j] * ((a - m) * (a - m)) : acc + wb[j] * a; }
                }
            }
            __syncthreads();
            red[tid] = acc;
            __syncthreads();
            if (part == 0) {
                float tot = 0.f;
                for (int pp = 0; pp < tpc; ++pp) tot = tot + red[pp * ncol + col];
                if (!phase) colmean[cb + col] = tot / W;
                else {
                    const float sd = sqrtf(tot / W);
                    const int ci = cb + col;
                    const float nsg = sm * old_sg + osm * sd;                          // cem_mpc.py:65
                    musig_b[ci] = sm * old_mu + osm * colmean[ci];                     // cem_mpc.py:64
                    musig_b[HA + ci] = nsg;
                    newsig[ci] = nsg;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        float ssum = 0.f;
        for (int i = 0; i < HA; ++i) ssum = ssum + newsig[i];
        const float mean_sigma = ssum / (float)HA;
        const int it = ctrl->iters - 1;                                                // the select in front has counted this iteration
        if (it >= 0 && it < p.I) p.stat[(size_t)prob * p.I + it] = W * W / Q;
        if (mean_sigma <= p.threshold) ctrl->done = 1;                                 // cem_mpc.py:66-67
    }
}

// the launch: one workgroup per problem
static inline hipError_t launch_refit_weighted(const RefitWeightedParams &p, int n_problems, hipStream_t stream)
{
    hipLaunchKernelGGL(cem_constraint_refit_kernel, dim3(n_problems), dim3(CEM_REFIT_THREADS), CEM_REFIT_LDS_BYTES(p.k, p.HA), stream, p);
    return hipGetLastError();
}
