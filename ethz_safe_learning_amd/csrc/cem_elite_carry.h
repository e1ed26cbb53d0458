// cem_elite_carry.h — elite carry-over (cem_planner_set_elite_carry): the best m elite sequences of an iteration are
// candidates 0 .. m - 1 of the next one, and — across_plans — of the next plan's first iteration, shifted by the steps that were executed.
// Two kernels around launches that stay what they were: the KEEP directly behind an iteration's select (and behind the weighted refit
// where that runs) copies the winners out of `actions` into a store the handle owns; the INJECT between the sampler launch
// (cem_sample_kernel) and the rollout launch of the next iteration overwrites rows 0 .. count - 1 of both action layouts from that store.
// The sampler has drawn those rows like any others (no candidate's Philox counters move) and the select ranks them like any others.
//
// Per problem: a store E[m][H][A] and an int32 count (0: nothing to inject).  The contract (include/cem_mpc.h; planner.keep_elites and
// planner.inject_elites restate it in NumPy, bit for bit):
//   keep, iteration `it`    acts iff ctrl.iters == it + 1 — the select in front counted this iteration; a select that left at once on
//                           `done` did not, and the select that SETS `done` still keeps.  The k entries of elite_idx are ordered by the
//                           key of the score the select ranked (cem_f2key: -0.0 and +0.0 tie, NaN below -inf), descending, ties by
//                           ascending candidate index; E[j] = actions[e_j] for the first m, exact copies; count = m.
//   inject, iteration `it`  leaves at once on `done` or count == 0.  s = (it == 0 ? shift : 0); for n < count, t < H - s, a < A:
//                           actions[n][t][a] = act_pad[n][t][pad_shift + a] = E[n][t + s][a].  Steps t >= H - s keep what the sampler drew
//                           for candidate n; the padding words of act_pad keep their zeros; nothing is clipped (stored values are clipped
//                           samples of the same box).
// Neither kernel does floating-point arithmetic: scores are compared as integer keys and actions move as words.
//
// Keep: one workgroup of 1024 threads per problem.  The k (key, index) pairs are staged in LDS (8 k bytes: 32 KB at the k = 4096
// limit).  Thread t ranks elites j = t, t + 1024, ... (at most four): it walks all k pairs — every lane of a wave reads the same pair, a
// broadcast, so the walk is free of bank conflicts — and counts those that precede j; the count is j's rank.  Behind a barrier the
// pairs are dead and the same LDS takes win[rank] = index for the ranks below m (a rank is held by exactly one elite: candidate indices
// are distinct); behind another all threads copy the m H A floats of the winners, thread after thread along the store, so both the
// reads (within a sequence) and the writes are coalesced.
// Inject: one thread per (row, step, action quad) of the store, grid.y the problem; `count` is read once.
//
// This header is what cem_capi.hip includes; the kernels are compiled in a translation unit of their own (cem_elite_carry.hip defines
// CEM_ELITE_CARRY_UNIT), as cem_noise_mix.h's is, so that the device code of cem_capi.hip stays what it was instruction for instruction.
#pragma once
#include "cem_device.h"

#define CEM_ELITE_MAX_K 4096
#define CEM_ELITE_THREADS 256            // the inject
#define CEM_ELITE_KEEP_THREADS 1024
#define CEM_ELITE_KEEP_PER_THREAD (CEM_ELITE_MAX_K / CEM_ELITE_KEEP_THREADS)
// dynamic LDS of the keep: (key, index) [k]
#define CEM_ELITE_KEEP_LDS_BYTES(k_) ((size_t)(k_) * 8)

struct EliteCarryParams {
    const float *scores;         // [problems][N] the scores the select ranked (keep)
    float *actions;              // [problems][N][H][A]: read by the keep, rows < count written by the inject
    float *act_pad;              // [problems][N][H][pad_floats]: action a of (n, t) at word pad_shift + a (inject)
    const CtrlBlock *ctrl;       // [problems]
    const int32_t *elite_idx;    // [problems][k] as the select stored them (keep)
    float *store;                // [problems][m][H][A]
    int32_t *count;              // [problems]
    int32_t N, k, m, H, A, it, shift, pad_shift, pad_floats;
};

// Weak: a library built from cem_capi.hip alone has no carry-over and cem_planner_set_elite_carry says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_elite_keep(const EliteCarryParams &p, int n_problems, hipStream_t st);
__attribute__((weak)) hipError_t launch_elite_inject(const EliteCarryParams &p, int n_problems, hipStream_t st);

#ifdef CEM_ELITE_CARRY_UNIT
__global__ __launch_bounds__(CEM_ELITE_KEEP_THREADS) void cem_elite_keep_kernel(const EliteCarryParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t elite_lds[];
    const int b = (int)blockIdx.x;
    if (p.ctrl[b].iters != p.it + 1) return;                 // workgroup-uniform: no barrier has been reached yet
    const int k = p.k, m = p.m, HA = p.H * p.A, tid = (int)threadIdx.x;
    uint2 *const pair = reinterpret_cast<uint2 *>(elite_lds);              // [k] (key, candidate index)
    int32_t *const win = reinterpret_cast<int32_t *>(elite_lds);           // [m] once the pairs are dead
    const uint32_t *const scores_b = reinterpret_cast<const uint32_t *>(p.scores) + (size_t)b * p.N;
    const int32_t *const elite_b = p.elite_idx + (size_t)b * k;
    for (int j = tid; j < k; j += CEM_ELITE_KEEP_THREADS) {
        // (an elite index is a candidate index by the select's contract; held to the population all the same: no read leaves the tensor)
        int e = elite_b[j]; e = (uint32_t)e < (uint32_t)p.N ? e : 0;
        // (the score is loaded as an integer and keyed by the selects' own function, cem_device.h: cem_f2key is cem_bits2key of the bits)
        pair[j] = make_uint2(cem_bits2key(scores_b[e]), (uint32_t)e);
    }
    __syncthreads();
    int rank[CEM_ELITE_KEEP_PER_THREAD], cand[CEM_ELITE_KEEP_PER_THREAD];
#pragma unroll
    for (int q = 0; q < CEM_ELITE_KEEP_PER_THREAD; ++q) {
        const int j = tid + q * CEM_ELITE_KEEP_THREADS;
        rank[q] = m; cand[q] = 0;                            // (no elite: no row)
        if (j < k) {
            const uint2 mine = pair[j];
            int before = 0;
            for (int i = 0; i < k; ++i) { const uint2 o = pair[i]; before += (o.x > mine.x || (o.x == mine.x && (int)o.y < (int)mine.y)) ? 1 : 0; }
            rank[q] = before; cand[q] = (int)mine.y;
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < CEM_ELITE_KEEP_PER_THREAD; ++q) if (rank[q] < m) win[rank[q]] = cand[q];
    __syncthreads();
    const float *const actions_b = p.actions + (size_t)b * p.N * HA;
    float *const store_b = p.store + (size_t)b * m * HA;
    for (int e = tid; e < m * HA; e += CEM_ELITE_KEEP_THREADS) {
        const int r = e / HA;
        // (every rank below m has its elite while the indices are distinct; were two equal, a rank would keep a stale word: held to the population)
        int w = win[r]; w = (uint32_t)w < (uint32_t)p.N ? w : 0;
        store_b[e] = actions_b[(size_t)w * HA + (e - r * HA)];
    }
    if (tid == 0) p.count[b] = m;
}

__global__ __launch_bounds__(CEM_ELITE_THREADS) void cem_elite_inject_kernel(const EliteCarryParams p)
{
    const int b = (int)blockIdx.y;
    if (p.ctrl[b].done) return;
    int c = p.count[b]; c = c < p.m ? c : p.m;               // (never more rows than the store has)
    const int H = p.H, A = p.A, AZ = (A + 3) >> 2, s = p.it == 0 ? p.shift : 0;
    const int q = (int)(blockIdx.x * CEM_ELITE_THREADS + threadIdx.x);
    const int z = q % AZ, t = (q / AZ) % H, n = q / (AZ * H);
    if (n >= c || t >= H - s) return;
    const float *src = p.store + (((size_t)b * p.m + n) * H + t + s) * A;
    float *nat = p.actions + (((size_t)b * p.N + n) * H + t) * A;
    float *pad = p.act_pad + (((size_t)b * p.N + n) * H + t) * p.pad_floats + p.pad_shift;
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int a = 4 * z + r; if (a < A) { const float v = src[a]; nat[a] = v; pad[a] = v; } }
}

hipError_t launch_elite_keep(const EliteCarryParams &p, int n_problems, hipStream_t st)
{
    hipLaunchKernelGGL(cem_elite_keep_kernel, dim3(n_problems), dim3(CEM_ELITE_KEEP_THREADS), CEM_ELITE_KEEP_LDS_BYTES(p.k), st, p);
    return hipGetLastError();
}

hipError_t launch_elite_inject(const EliteCarryParams &p, int n_problems, hipStream_t st)
{
    const int total = p.m * p.H * ((p.A + 3) / 4);
    hipLaunchKernelGGL(cem_elite_inject_kernel, dim3((total + CEM_ELITE_THREADS - 1) / CEM_ELITE_THREADS, n_problems), dim3(CEM_ELITE_THREADS), 0, st, p);
    return hipGetLastError();
}
#endif
