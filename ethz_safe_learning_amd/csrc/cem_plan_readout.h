// cem_plan_readout.h — the plan read-out (cem_planner_set_plan_readout): what the optimiser knew about the sequence it
// chose, copied out of the workspace before the next iteration's rollout overwrites it.  One kernel, the TRACKER, directly behind an
// iteration's select (behind the weighted refit and the elite keep where those run: the keep only reads `actions`, so the order between
// the two is free — the tracker is the LAST launch of enqueue_select, which keeps every earlier launch where it was).  No other kernel
// changes, none reads what the tracker writes.
//
// Per problem a block of 4 + H A + P + H words in an allocation the handle owns:
//   word 0 score (fp32)      the best-so-far score, a copy of ctrl.best_score               (initially -inf)
//   word 1 candidate (int32) its index in the population of the iteration that found it     (initially -1)
//   word 2 iteration (int32) that iteration                                                 (initially -1)
//   word 3 flags (int32)     bit 0: an update was signalled and no elite matched (never set by a select of this library)
//   sequence [H][A] fp32     the candidate's row of `actions`, exact copy                   (initially zeros)
//   particle_returns [P]     ret[q N + candidate], q = 0 .. P - 1, exact copies             (initially zeros)
//   cost_counts [H] int32    at step t the number of particles q with costs[t][q N + candidate] != 0; -1 everywhere on handles whose
//                            rollout stores no cost bytes                                   (initially 0 / -1)
// N is the population of the iteration that found the candidate (cem_population.h).  The contract (include/cem_mpc.h; planner.track_best
// restates it in NumPy, bit for bit), launch `it` of a plan:
//   reset    it == 0 puts the block into its initial state, whether or not the select in front counted the iteration: a batch row that
//            is not live keeps iters == 0 and must read "nothing found", not the previous plan's block.
//   gate     the launch goes on iff ctrl.iters == it + 1 — the keep's rule (cem_elite_carry.h): a select that left at once on `done` did
//            not count the iteration, the select that SETS `done` did.
//   update   iff key(ctrl.best_score) > key(block.score), keys as the selects rank scores (cem_bits2key).  Neither is a NaN, the two zeros
//            share a key: this is the fp32 comparison best_score > score — the select's own strict test (cem_select_kernel: `better`), of
//            which ctrl.best_score changes iff it holds, so that an equal score in a later iteration is no update.
//   which    the lowest candidate index among the k entries of elite_idx whose score has ctrl.best_score's key.  The select's winner is
//            the elite of maximum score, exact ties to the lowest candidate index (cem_select_kernel: the compaction walk keeps a thread's
//            first maximum, threads and waves combine on (score, index)); ctrl.best_score is that maximum, so the elites that compare
//            equal to it are exactly the maximum's ties and the lowest of them is the winner.  No re-ranking.  (With NaN among the
//            elites — fewer than k scores that are numbers — the select's walk can settle on a smaller score than the maximum; the rule
//            here still names an elite of exactly the score the select stored.)  No match: flag bit 0, the rest of the block stays.
//   copy     the sequence, the P returns, the per-step counts of non-zero cost bytes.
// No floating-point arithmetic — scores are compared as integer keys, everything else moves as words or is counted — and no atomics:
// the minimum over the workgroup goes through wave shuffles and four LDS words.  Every index read from memory is held to its tensor.
//
// One workgroup of 256 threads per problem: the block is at most a few hundred words (H A + P + H; the shipped shapes: 30 x 2 + 20 + 30),
// the k elite entries are one or two strided trips, and the counts take a wave per step — lane q loads particle q's byte (two trips up
// to the 128 particles the setter admits), a ballot counts them.  Four waves are as many as have work; every word of the block is
// written at most once per launch, by one thread, so the reset and the copy cannot race.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_plan_readout.hip defines
// CEM_PLAN_READOUT_UNIT), as cem_elite_carry.h's are, so that the device code of cem_capi.hip stays what it was instruction for instruction.
#pragma once
#include "cem_device.h"

#define CEM_READOUT_THREADS 256
#define CEM_READOUT_MAX_P 128            // the particle objectives' cap (cem_score.h: CEM_TAIL_MAX_P)
#define CEM_READOUT_HEAD 4               // score, candidate, iteration, flags
// words of one problem's block
#define CEM_READOUT_WORDS(H_, A_, P_) ((size_t)CEM_READOUT_HEAD + (size_t)(H_) * (A_) + (size_t)(P_) + (size_t)(H_))

struct PlanTrackParams {
    const float *scores;         // [problems][N] the scores the select ranked
    const float *actions;        // [problems][N][H][A]
    const float *ret;            // [problems][P][N]
    const uint8_t *costs;        // [problems][H][P][N], or null: the rollout stores no cost bytes
    const CtrlBlock *ctrl;       // [problems]
    const int32_t *elite_idx;    // [problems][k] as the select stored them
    uint32_t *block;             // [problems][stride]
    int32_t N, k, H, A, P, it, stride;
};

// Weak: a library built from cem_capi.hip alone has no read-out and cem_planner_set_plan_readout says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_plan_track(const PlanTrackParams &p, int n_problems, hipStream_t st);

#ifdef CEM_PLAN_READOUT_UNIT
__global__ __launch_bounds__(CEM_READOUT_THREADS) void cem_plan_track_kernel(const PlanTrackParams p)
{
    __shared__ int32_t wave_min[CEM_READOUT_THREADS / 64];
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = p.N, H = p.H, P = p.P, HA = p.H * p.A;
    uint32_t *const blk = p.block + (size_t)b * p.stride;
    const CtrlBlock *const ctrl = p.ctrl + b;
    const bool first = p.it == 0;
    const uint32_t best = __float_as_uint(ctrl->best_score);
    const uint32_t flags = first ? 0u : blk[3];
    // (the block's score is read before anything of the block is written; 0xff800000: -inf)
    const bool update = ctrl->iters == p.it + 1 && cem_bits2key(best) > cem_bits2key(first ? 0xff800000u : blk[0]);
    if (!first && !update) return;                           // workgroup-uniform: no barrier has been reached yet

    int cand = 0x7fffffff;
    if (update) {
        const uint32_t *const scores_b = reinterpret_cast<const uint32_t *>(p.scores) + (size_t)b * N;
        const int32_t *const elite_b = p.elite_idx + (size_t)b * p.k;
        const uint32_t want = cem_bits2key(best);
        for (int j = tid; j < p.k; j += CEM_READOUT_THREADS) {
            // (an elite index is a candidate index by the select's contract; held to the population all the same: no read leaves the tensor)
            int e = elite_b[j]; e = (uint32_t)e < (uint32_t)N ? e : 0;
            if (cem_bits2key(scores_b[e]) == want) cand = e < cand ? e : cand;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) { const int o = __shfl_xor(cand, d); cand = o < cand ? o : cand; }
    }
    if (lane == 0) wave_min[wv] = cand;
    __syncthreads();
#pragma unroll
    for (int w = 0; w < CEM_READOUT_THREADS / 64; ++w) { const int o = wave_min[w]; cand = o < cand ? o : cand; }
    const bool found = cand != 0x7fffffff;                   // (workgroup-uniform from here; found implies update)
    if (!first && !found) { if (tid == 0) blk[3] = flags | 1u; return; }

    if (tid == 0) {
        blk[0] = found ? best : 0xff800000u;
        blk[1] = found ? (uint32_t)cand : 0xffffffffu;
        blk[2] = found ? (uint32_t)p.it : 0xffffffffu;
        blk[3] = flags | ((update && !found) ? 1u : 0u);
    }
    const int c = found ? cand : 0;                          // (below N: every match was held to the population)
    uint32_t *const seq = blk + CEM_READOUT_HEAD, *const pret = seq + HA, *const cnt = pret + P;
    const uint32_t *const act_c = reinterpret_cast<const uint32_t *>(p.actions) + ((size_t)b * N + c) * HA;
    for (int e = tid; e < HA; e += CEM_READOUT_THREADS) seq[e] = found ? act_c[e] : 0u;
    const uint32_t *const ret_c = reinterpret_cast<const uint32_t *>(p.ret) + (size_t)b * P * N + c;
    for (int q = tid; q < P; q += CEM_READOUT_THREADS) pret[q] = found ? ret_c[(size_t)q * N] : 0u;
    if (!p.costs) {
        for (int t = tid; t < H; t += CEM_READOUT_THREADS) cnt[t] = 0xffffffffu;
    } else if (!found) {
        for (int t = tid; t < H; t += CEM_READOUT_THREADS) cnt[t] = 0u;
    } else {
        // a wave per step: lane q and lane q + 64 of the second trip hold particle q's byte, the ballots count the non-zero ones
        const uint8_t *const costs_c = p.costs + (size_t)b * H * P * N + c;
        for (int t = wv; t < H; t += CEM_READOUT_THREADS / 64) {
            const uint8_t *const row = costs_c + (size_t)t * P * N;
            uint32_t n = 0;
            for (int q0 = 0; q0 < P; q0 += 64) {
                const int q = q0 + lane;
                const bool nz = q < P && row[(size_t)q * N] != 0;
                n += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(nz));
            }
            if (lane == 0) cnt[t] = n;
        }
    }
}

hipError_t launch_plan_track(const PlanTrackParams &p, int n_problems, hipStream_t st)
{
    hipLaunchKernelGGL(cem_plan_track_kernel, dim3(n_problems), dim3(CEM_READOUT_THREADS), 0, st, p);
    return hipGetLastError();
}
#endif
