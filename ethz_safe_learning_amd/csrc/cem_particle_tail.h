// cem_particle_tail.h — the risk-averse particle objective (cem_mpc.h, cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL):
// a candidate's score is the mean of the m SMALLEST of its P particle returns (CVaR at level m / P; m = 1: the worst particle) instead
// of the reference's mean over all of them (mpc_policy.py:38-39).  The returns come from the unchanged rollout kernels (or from
// cem_objective_kernel for the standalone op); what is left is this reduction, launched where cem_reduce_kernel would be.
//   value[n] = (((0.f + r_(0)) + r_(1)) + ... + r_(m-1)) / (float)m,  r_(i) the particle returns of candidate n in ascending order of
//   (return, particle index): equal returns go in particle order, -0.f == 0.f.  NaN returns are outside the contract.
// On a CEM_VARIANT_SAFE handle the Beta filter is cem_reduce_kernel's, applied to this value: score = value - (unsafe ? 1 : 0) * 100.
// P <= CEM_TAIL_MAX_P = 128 (eight particles per wave held in registers, P x 64 returns in LDS); beyond that the setter answers
// CEM_ERR_UNSUPPORTED.  Included from cem_capi.hip behind cem_device.h (CtrlBlock).
#pragma once

struct ConstraintTailParams {
    const float *ret;            // [P][Nloc] per-particle returns of the last rollout
    const uint8_t *costs;        // [H][P][Nloc] masked per-step cost (variant 1), or null
    float *scores;               // [Nloc]
    const CtrlBlock *ctrl;
    int32_t Nloc, P, H, m, variant, check_done;
    float alpha, beta, thr;
    uint32_t *zero; int32_t zero_n;        // words block 0 clears for the multi-workgroup select that follows (as ReduceParams::zero), or null
    // batched plans: blockIdx.y is the problem; its ret / costs / scores are the next [P][Nloc] / [H][P][Nloc] / [Nloc] slices, its
    // control block ctrl[blockIdx.y]
};

#define CEM_TAIL_THREADS 1024
#define CEM_TAIL_MAX_P 128
// dynamic LDS, 32-bit words: unsafe_w [16][64], cnt_s [16][64], ret_s [P][64]  (P = 45: 19.25 KiB, P = 128: 40 KiB)
#define CEM_TAIL_LDS_BYTES(P) ((size_t)(2 * 16 * 64 + (P) * 64) * 4)

// cem_reduce_kernel's per-step Beta counts (safe_cem_mpc.py:90-96,110-120), its arithmetic operation for operation: the OR over this
// wave's steps of (alpha + count_t) / ((alpha + beta) + P) > thr.  Counts are integers (exact, order-free).  Every wave of the block
// calls it (it holds barriers).
__device__ __forceinline__ int32_t cem_tail_unsafe(const ConstraintTailParams &p, const uint8_t *costs, int nn, int w, int lane, uint32_t *cnt_s)
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
        cnt_s[w * 64 + lane] = 0u;
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
            if (wpt > 1) atomicAdd(&cnt_s[t * 64 + lane], cnt); else cnt_s[t * 64 + lane] = cnt;
        }
        __syncthreads();
        if (w < H) unsafe = ((p.alpha + (float)cnt_s[w * 64 + lane]) / denom <= p.thr) ? 0 : 1;
    }
    return unsafe;
}

// One block = 64 candidates (one per lane) x 16 waves, the load shape of cem_reduce_kernel.  Wave w owns particles w, w + 16, ...
// (J of them at most, in registers): it loads them (coalesced over the lanes), leaves them in the LDS column of its lane, and after a
// barrier ranks each against all P of the column by counting the particles that come before it in (return, index) order — a permutation
// of 0 .. P-1, so after a second barrier those of rank < m go to row `rank` of the same column and no two writes meet.  Wave 0 then adds
// rows 0 .. m-1 in order, divides, applies the Beta filter and stores.  Every LDS access is one dword per lane at bank lane % 32: no conflicts.
template <int J>
__device__ __forceinline__ void cem_tail_body(const ConstraintTailParams &p, uint32_t *lds)
{
    int32_t *const unsafe_w = (int32_t *)lds;
    uint32_t *const cnt_s = lds + 16 * 64;
    float *const ret_s = (float *)(lds + 2 * 16 * 64);
    const int b = (int)blockIdx.y;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + lane;
    const bool live = n < p.Nloc;
    const int nn = live ? n : p.Nloc - 1;
    const int P = p.P, m = p.m;
    const float *const ret = p.ret + (size_t)b * P * p.Nloc;
    float v[J];
#pragma unroll
    for (int j = 0; j < J; ++j) { const int q = w + 16 * j; v[j] = ret[(size_t)(q < P ? q : 0) * p.Nloc + nn]; }   // (clamped: the loads are unconditional)
    if (p.variant == 1) unsafe_w[w * 64 + lane] = cem_tail_unsafe(p, p.costs + (size_t)b * p.H * P * p.Nloc, nn, w, lane, cnt_s);
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P) ret_s[(w + 16 * j) * 64 + lane] = v[j];
    __syncthreads();
    int rk[J];
#pragma unroll
    for (int j = 0; j < J; ++j) rk[j] = 0;
    for (int q = 0; q < P; ++q) {
        const float x = ret_s[q * 64 + lane];
#pragma unroll
        for (int j = 0; j < J; ++j) rk[j] += (x < v[j] || (x == v[j] && q < w + 16 * j)) ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) if (w + 16 * j < P && rk[j] < m) ret_s[rk[j] * 64 + lane] = v[j];
    __syncthreads();
    if (w != 0 || !live) return;
    float sum = 0.f;
    for (int i = 0; i < m; ++i) sum = sum + ret_s[i * 64 + lane];
    float score = sum / (float)m;
    if (p.variant == 1) {
        int32_t u = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) u |= unsafe_w[i * 64 + lane];
        score = score - (u ? 1.0f : 0.0f) * 100.0f;
    }
    p.scores[(size_t)b * p.Nloc + n] = score;
}

__global__ __launch_bounds__(CEM_TAIL_THREADS) void cem_constraint_tail_kernel(const ConstraintTailParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t cem_tail_lds[];
    const int b = (int)blockIdx.y;
    if (p.check_done && p.ctrl[b].done) return;
    if (p.zero && blockIdx.x == 0 && b == 0) for (int i = threadIdx.x; i < p.zero_n; i += CEM_TAIL_THREADS) p.zero[i] = 0u;
    const int per_wave = (p.P + 15) >> 4;                              // particles the busiest wave owns (uniform)
    if (per_wave <= 1) cem_tail_body<1>(p, cem_tail_lds);
    else if (per_wave <= 2) cem_tail_body<2>(p, cem_tail_lds);
    else if (per_wave <= 4) cem_tail_body<4>(p, cem_tail_lds);
    else cem_tail_body<8>(p, cem_tail_lds);
}

// the launch: grid.x = blocks of 64 candidates, grid.y = problems of a batched plan
static inline hipError_t launch_constraint_tail(const ConstraintTailParams &p, int n_problems, hipStream_t stream)
{
    hipLaunchKernelGGL(cem_constraint_tail_kernel, dim3((p.Nloc + 63) / 64, n_problems), dim3(CEM_TAIL_THREADS), CEM_TAIL_LDS_BYTES(p.P), stream, p);
    return hipGetLastError();
}
