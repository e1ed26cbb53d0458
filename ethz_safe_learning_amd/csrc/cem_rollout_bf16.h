// cem_rollout_bf16.h — the reduced-precision rollout (config field `precision` = CEM_PRECISION_BF16; opt-in, never the default):
// the operands of every dense stage rounded to bf16, once, and nothing else.
//
// The arithmetic (the contract; planner.bf16_reference_forward restates it in NumPy):
//   weights    rounded to bf16, round to nearest even (cem_rn_bf16_bits), when they are packed — host and device packers alike;
//   inputs     of every dense stage rounded the same way by the wave that publishes them (v_cvt_pk_bf16_f32): the scaled layer-0 input,
//              observation and action features alike, and every post-ReLU hidden activation;
//   products   exact in the fp32 accumulator of v_mfma_f32_16x16x32_bf16; sums fp32, starting from the fp32 bias;
//   the rest   — state, (x - min) * (1 / delta), head outputs, softplus / + 1e-4 / sqrt, s += mu + sigma eps, Philox, scorer terms,
//              reward / cost / done bookkeeping — is the fp32 code of the other kernels (cem_rollout_common.h where it lives there).
// Finite inputs below the largest bf16; units <= 128 and relu, like the split kernel.
//
// Structure: the one-plane variant of the chunked tile (cem_rollout_chunked.h's body, shared with the split kernel): wave w keeps
// its output blocks 2w, 2w + 1 of a hidden layer, rounded, as its own K = 32 chunk of the next stage; the other chunks travel
// through LDS as ONE bf16 plane, [2 buffers][RC][4 chunks][64 lanes][16 B]; weights stream from a per-wave image of 2 KB groups
// ({a, b} output block x [64 lanes][8 bf16]) in the split kernel's visiting order (cem_split_perm).  One MFMA per (chunk, output
// block) where the split kernel issues six, one plane where it moves three, one conversion where it splits.  A stage's LDS chunks are
// all read right behind its barrier (at most 12 RC VGPRs): a chunk's MFMAs are 32 RC cycles, shorter than an LDS round trip.
// Whole-horizon tiles only (no floating segments); MODE 1 also serves cem_unfold_sequences (trajectory / head-moment outputs).
//
// A translation unit of its own (cem_rollout_bf16.hip defines CEM_ROLLOUT_BF16_UNIT): cem_capi.hip sees the launcher's declaration
// alone, so none of its kernels is compiled beside this one.
#pragma once
#include "cem_device.h"
#include "cem_rollout_split.h"

// Weight ring depth: CEM_BF16_RING slots of 8 VGPRs, RING - 1 groups ahead of the MFMAs.  Every stage must be a multiple of RING chunks
// long for the slot of a chunk to be a compile-time constant, so a ring of 4 pads the two-chunk layer 0 of the obs + act <= 64 family
// with two zero-weight chunks (+11 % weight bytes and MFMAs at depth 4); 2 pads nothing.  Measured 2 vs 4, launch ms on one device
// (profiles/bf16_rollout_isa.txt): B1 0.0656 vs 0.0618, B2 0.104 vs 0.105, B3 0.702 vs 0.731, B4 0.434 vs 0.567 (16 more VGPRs cost the
// four-chunk tile of the obs + act > 64 family its second resident workgroup).
#ifndef CEM_BF16_RING
#define CEM_BF16_RING 2
#endif

// mode 0: planning; mode 1: caller-supplied noise tensors, trajectory and head-moment outputs.  Weak: a library built from cem_capi.hip
// alone (the host sanitizer build) has no bf16 rollout and says so (CEM_ERR_UNSUPPORTED at create).
__attribute__((weak)) hipError_t launch_rollout_bf16(int rc, int nfw, int mode, const RolloutParams &p, int n_tiles, hipStream_t st);

#ifdef CEM_ROLLOUT_BF16_UNIT

__device__ __forceinline__ int cem_bf16_off(const int c_rc, const int chunk, const int lane) { return ((c_rc * CEM_SPLIT_CHUNKS + chunk) * 64 + lane) * 16; }

__device__ __forceinline__ unsigned cem_bf16_pair(const float x0, const float x1)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f2){x0, x1}, cem_bf2));
}

typedef ChunkRing<2, CEM_BF16_RING> BRing;            // (cem_rollout_split.h) over the stream of 2 KB groups

// One dense stage: acc{0,1}[c] += W^T x over the stage's chunks.  OWN: chunk 0 of the visiting order is the wave's own (in registers)
// and the barrier that publishes the other waves' chunks comes after its MFMAs.  XMODE as in cem_mfma_stage.
template <int RC, int NCH, bool OWN, int XMODE>
__device__ __forceinline__ void cem_bf16_stage(f4 (&acc0)[RC], f4 (&acc1)[RC], const cem_u4 (&own)[RC], BRing &wq, const char *smem, const int xr,
                                               const int lane, const int w)
{
    static_assert(NCH % CEM_BF16_RING == 0, "stage lengths must keep the ring phase");
    constexpr int FL = OWN ? 1 : 0;                        // visiting position of the first chunk that comes from LDS
    cem_u4 bp[NCH][RC];
#pragma unroll
    for (int P = 0; P < NCH; ++P) {
        wq.ld(wq.slot[(P + CEM_BF16_RING - 1) % CEM_BF16_RING], wq.pos);       // the group RING - 1 chunks ahead (possibly the next stage's)
        wq.pos = (wq.pos + 1 == wq.n) ? 0 : wq.pos + 1;
        __builtin_amdgcn_sched_barrier(0);
        const cem_u4 (&g)[2] = wq.slot[P % CEM_BF16_RING];
        if (OWN && P == 0) {
#pragma unroll
            for (int c = 0; c < RC; ++c) { acc0[c] = CEM_MFMA_BF(g[0], own[c], acc0[c]); acc1[c] = CEM_MFMA_BF(g[1], own[c], acc1[c]); }
        }
        if (P == 0) {
            if (XMODE == CEM_X_EXCHANGE) __syncthreads();
#pragma unroll
            for (int Q = FL; Q < NCH; ++Q) {
                const int F = OWN ? cem_split_perm(w, Q) : Q;
#pragma unroll
                for (int c = 0; c < RC; ++c) bp[Q][c] = *reinterpret_cast<const cem_u4 *>(smem + xr + cem_bf16_off(c, F, lane));
            }
            if (OWN) continue;
        }
#pragma unroll
        for (int c = 0; c < RC; ++c) { acc0[c] = CEM_MFMA_BF(g[0], bp[P][c], acc0[c]); acc1[c] = CEM_MFMA_BF(g[1], bp[P][c], acc1[c]); }
    }
}

// The tile (cem_rollout_tile_bf16) is cem_rollout_chunked.h's body with one plane, rounded by the publishing wave:
#define CEM_CHUNKED_TILE cem_rollout_tile_bf16
#define CEM_CHUNKED_PLANES 1
#define CEM_CHUNKED_RING CEM_BF16_RING
#define CEM_CHUNKED_STAGE cem_bf16_stage
#define CEM_CHUNKED_OWN(OWN_, RC_) cem_u4 OWN_[RC_]; \
    _Pragma("unroll") for (int c = 0; c < (RC_); ++c) OWN_[c] = (cem_u4){0u, 0u, 0u, 0u}
// the scaled input block FO_ of row chunk C_ goes to LDS rounded: 4 bf16 per lane (its half of the lane's 16 bytes)
#define CEM_CHUNKED_PUBLISH_X(SMEM_, XW_, LANE_, X_, FO_, C_) do { \
        *reinterpret_cast<cem_u2 *>((SMEM_) + (XW_) + cem_bf16_off((C_), (FO_) >> 1, LANE_) + 8 * ((FO_) & 1)) = \
            (cem_u2){cem_bf16_pair((X_)[0], (X_)[1]), cem_bf16_pair((X_)[2], (X_)[3])}; } while (0)
// round, keep as the own chunk and publish: 4 v_cvt_pk_bf16_f32 per 8 activations
#define CEM_CHUNKED_PUBLISH_H(SMEM_, XW_, LANE_, W_, H0_, H1_, OWN_, C_) do { \
        OWN_[C_] = (cem_u4){cem_bf16_pair(H0_[0], H0_[1]), cem_bf16_pair(H0_[2], H0_[3]), cem_bf16_pair(H1_[0], H1_[1]), cem_bf16_pair(H1_[2], H1_[3])}; \
        *reinterpret_cast<cem_u4 *>((SMEM_) + (XW_) + cem_bf16_off(C_, W_, LANE_)) = OWN_[C_]; } while (0)
#include "cem_rollout_chunked.h"

template <int RC, int NFW, int MODE>
__global__ __launch_bounds__(256) void cem_rollout_bf16_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_tile_sample_actions(p, (int)blockIdx.x, 0, p.H, true, MODE == 1);
    cem_rollout_tile_bf16<RC, NFW, MODE>(p, smem, (int)blockIdx.x);
}

#endif  // CEM_ROLLOUT_BF16_UNIT
