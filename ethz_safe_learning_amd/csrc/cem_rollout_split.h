// cem_rollout_split.h — the rollout with every fp32 product formed on the bf16 matrix pipe from EXACT three-way splits
// (config field `precision` = CEM_PRECISION_SPLIT_BF16X3; opt-in, never the default).
//
// An fp32 number is the exact sum of three bf16 numbers, x = x0 + x1 + x2 (8 significand bits each: x0 = RN(x), x1 = RN(x - x0),
// x2 = x - x0 - x1, round to nearest even).  A product w * x is then the sum of nine bf16 x bf16 products, each exact in the fp32
// accumulator of v_mfma_f32_16x16x32_bf16; the six with i + j <= 2 carry everything down to 2^-23 of the product — the scale of
// one fp32 rounding — and the other three are dropped.  Six bf16 MFMAs of K = 32 replace eight fp32
// MFMAs of K = 4 per (two input blocks x one output block): 96 matrix-pipe cycles instead of 256.  (A wave's VALU work still adds
// to its MFMA time — interleaving the publish with the next row-chunk's MFMAs gained nothing, profiles/r03_split_tile_sizes.txt —
// so the split itself, 44 VALU per 8 values, is part of the price.)  Not bit-identical to the fp32 kernels (the products are summed
// inside the MFMA, 32 at a time), same error scale; parity is measured against the same oracle at the same tolerances
// (tests/test_gpu_split.py).
//
// Structure: cem_rollout_tile's — 4 waves per tile of 16 RC rows of one member for the whole horizon, wave w computes output blocks
// 2w, 2w + 1 of a hidden layer and keeps them, SPLIT, as its own K = 32 input chunk of the next stage; the other chunks travel through
// LDS as three bf16 planes; weights stream from a per-wave image of 6 KB groups (chunk x {a, b} output block x 3 planes) in visiting
// order.  The tile around the stages is cem_rollout_chunked.h's, shared with the one-plane kernel (cem_rollout_bf16.h); this header
// keeps the split primitives, the LDS offsets, the ring, the stage and what the shared tile takes from them (the CEM_CHUNKED_* hooks).
// Whole-horizon tiles only (no floating segments); MODE 1 also serves cem_unfold_sequences (trajectory / head-moment outputs).
#pragma once
#include "cem_device.h"

typedef __bf16 cem_bf8 __attribute__((ext_vector_type(8)));
typedef unsigned int cem_u2 __attribute__((ext_vector_type(2)));
#define CEM_MFMA_BF(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(cem_bf8, (a)), __builtin_bit_cast(cem_bf8, (b)), (c), 0, 0, 0)
#define CEM_SPLIT_CHUNKS 4                   // K = 32 chunks of a 128-feature layer

// x -> (x0, x1, x2) as bit patterns whose upper halves are the bf16 pieces: x0 = RN(x), x1 = RN(x - x0), x2 = x - x0 - x1 with RN =
// round to nearest even at 8 significand bits (what v_cvt_pk_bf16_f32 does).  Both subtractions are exact and x2 has at most 8
// significant bits, so x = x0 + x1 + x2 exactly (|x| below the largest bf16, 3.39e38) with |x1| <= 2^-8 |x|, |x2| <= 2^-16 |x|:
// the three dropped products are below 2^-23 of w x.  (A truncation split is exact too, but its pieces only shrink by 2^-7 each:
// the dropped terms reach 2^-21; tests/test_split_cpu.py.)  Host version (weights); the device splits pairs, below.
__host__ __device__ inline unsigned cem_rn_bf16_bits(const float x)
{
    union { float f; unsigned u; } v; v.f = x;
    return (v.u + 0x7FFFu + ((v.u >> 16) & 1u)) & 0xFFFF0000u;
}
__host__ __device__ inline void cem_split3_bits(const float x, unsigned &a0, unsigned &a1, unsigned &a2)
{
    union { float f; unsigned u; } t, r1, r2;
    a0 = cem_rn_bf16_bits(x);
    t.u = a0; r1.f = x - t.f; a1 = cem_rn_bf16_bits(r1.f);
    t.u = a1; r2.f = r1.f - t.f; a2 = r2.u;                 // exactly a bf16 value already
}

typedef __bf16 cem_bf2 __attribute__((ext_vector_type(2)));
// two values -> their three pieces, one packed word per plane: 11 VALU instructions (3 v_cvt_pk_bf16_f32, 4 shifts / masks, 4 subtractions)
__device__ __forceinline__ void cem_split_pair(const float x0, const float x1, unsigned &p0, unsigned &p1, unsigned &p2)
{
    p0 = __builtin_bit_cast(unsigned, __builtin_convertvector((f2){x0, x1}, cem_bf2));
    const float r1l = x0 - __uint_as_float(p0 << 16), r1h = x1 - __uint_as_float(p0 & 0xFFFF0000u);
    p1 = __builtin_bit_cast(unsigned, __builtin_convertvector((f2){r1l, r1h}, cem_bf2));
    const float r2l = r1l - __uint_as_float(p1 << 16), r2h = r1h - __uint_as_float(p1 & 0xFFFF0000u);
    p2 = __builtin_bit_cast(unsigned, __builtin_convertvector((f2){r2l, r2h}, cem_bf2));
}
// 8 values (two accumulator quads: features 4q..4q+3 of two 16-feature blocks) -> three planes of 8 bf16
__device__ __forceinline__ void cem_split8(const f4 x0, const f4 x1, cem_u4 (&p)[3])
{
    unsigned a[4], b[4], c[4];
    cem_split_pair(x0[0], x0[1], a[0], b[0], c[0]);
    cem_split_pair(x0[2], x0[3], a[1], b[1], c[1]);
    cem_split_pair(x1[0], x1[1], a[2], b[2], c[2]);
    cem_split_pair(x1[2], x1[3], a[3], b[3], c[3]);
    p[0] = (cem_u4){a[0], a[1], a[2], a[3]}; p[1] = (cem_u4){b[0], b[1], b[2], b[3]}; p[2] = (cem_u4){c[0], c[1], c[2], c[3]};
}
// 4 values (one feature quad of one block) -> three planes of 4 bf16
__device__ __forceinline__ void cem_split4(const f4 x, cem_u2 (&p)[3])
{
    unsigned a[2], b[2], c[2];
    cem_split_pair(x[0], x[1], a[0], b[0], c[0]);
    cem_split_pair(x[2], x[3], a[1], b[1], c[1]);
    p[0] = (cem_u2){a[0], a[1]}; p[1] = (cem_u2){b[0], b[1]}; p[2] = (cem_u2){c[0], c[1]};
}

// chunk visited at position phi of a hidden / heads stage by wave w: its own chunk (blocks 2w, 2w + 1) first, the others ascending
__host__ __device__ inline int cem_split_perm(int w, int phi) { return phi == 0 ? w : (phi - 1 < w ? phi - 1 : phi); }

// LDS: [2 buffers][RC][4 chunks][3 planes][64 lanes][16 B]; a lane's 16 bytes = 4 bf16 of block 2c, 4 bf16 of block 2c + 1
__device__ __forceinline__ int cem_split_off(const int c_rc, const int chunk, const int plane, const int lane)
{
    return (((c_rc * CEM_SPLIT_CHUNKS + chunk) * 3 + plane) * 64 + lane) * 16;
}

// Weight ring over a wave's stream of groups of NL KB, [a planes][b planes], a plane = [64 lanes][8 bf16] (6 KB here, 2 KB in
// cem_rollout_bf16.h): RING slots, RING - 1 groups ahead of the MFMAs; every stage is a multiple of RING chunks long, so the slot of a
// stage's chunk phi is the compile-time constant phi % RING (with RING 4 the two-chunk layer 0 of the obs+act <= 64 family is padded
// with two zero-weight chunks: cem_chunked_l0_chunks, host and device).
#ifndef CEM_SPLIT_RING
#define CEM_SPLIT_RING 2                       // measured 2 vs 4 (same box): B1 0.123 vs 0.133 ms, B2 0.358 vs 0.510, B3 2.93 vs 3.12, B4 1.60 vs 1.86 (48 more VGPRs cost a resident workgroup)
#endif
template <int NL, int RING>
struct ChunkRing {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff, n, pos;
    cem_u4 slot[RING][NL];
    __device__ __forceinline__ void ld(cem_u4 (&s)[NL], const int g) const
    {
#pragma unroll
        for (int i = 0; i < NL; ++i) s[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, g * (NL * 1024) + i * 1024, 0);
    }
    __device__ __forceinline__ void init(const f4 *b, const int lane_, const int n_)
    {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<f4 *>(b), 0, n_ * (NL * 1024), 0x00020000);
        voff = lane_ * 16; n = n_;
#pragma unroll
        for (int i = 0; i < RING - 1; ++i) ld(slot[i], i % n_);
        pos = (RING - 1) % n_;
    }
};
typedef ChunkRing<6, CEM_SPLIT_RING> SRing;

// One dense stage: acc{0,1}[c] += sum over the stage's chunks of the six split products.  OWN: chunk 0 of the visiting order is the
// wave's own (planes in registers) and the barrier that publishes the other waves' chunks comes after its MFMAs.  XMODE as in
// cem_mfma_stage (exchange: barrier inside; re-read: the input was published and waited for by an earlier stage).
template <int RC, int NCH, bool OWN, int XMODE>
__device__ __forceinline__ void cem_split_stage(f4 (&acc0)[RC], f4 (&acc1)[RC], const cem_u4 (&own)[RC][3], SRing &wq, const char *smem, const int xr,
                                                const int lane, const int w)
{
    static_assert(NCH % CEM_SPLIT_RING == 0, "stage lengths must keep the ring phase");
    constexpr int FL = OWN ? 1 : 0;                        // visiting position of the first chunk that comes from LDS
    cem_u4 bp[2][RC][3];                                   // B planes of the chunk in use and of the next one
    // the six products of one chunk for both output blocks, smallest terms first: (weight plane, activation plane)
    // (2,0) (1,1) (0,2) | (1,0) (0,1) (0,0); HALF 0 / 1 = the first / last three (the own chunk straddles the barrier)
#define CEM_SPLIT_PRODUCTS(G_, B0_, B1_, B2_, C_, HALF_) do { \
        if ((HALF_) != 1) { \
            acc0[C_] = CEM_MFMA_BF((G_)[2], B0_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[5], B0_, acc1[C_]); \
            acc0[C_] = CEM_MFMA_BF((G_)[1], B1_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[4], B1_, acc1[C_]); \
            acc0[C_] = CEM_MFMA_BF((G_)[0], B2_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[3], B2_, acc1[C_]); } \
        if ((HALF_) != 0) { \
            acc0[C_] = CEM_MFMA_BF((G_)[1], B0_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[4], B0_, acc1[C_]); \
            acc0[C_] = CEM_MFMA_BF((G_)[0], B1_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[3], B1_, acc1[C_]); \
            acc0[C_] = CEM_MFMA_BF((G_)[0], B0_, acc0[C_]); acc1[C_] = CEM_MFMA_BF((G_)[3], B0_, acc1[C_]); } } while (0)
#define CEM_SPLIT_READ(Q_) do { const int F_ = OWN ? cem_split_perm(w, (Q_)) : (Q_); \
        _Pragma("unroll") for (int c = 0; c < RC; ++c) \
            _Pragma("unroll") for (int j = 0; j < 3; ++j) \
                bp[(Q_) & 1][c][j] = *reinterpret_cast<const cem_u4 *>(smem + xr + cem_split_off(c, F_, j, lane)); } while (0)
#pragma unroll
    for (int P = 0; P < NCH; ++P) {
        wq.ld(wq.slot[(P + CEM_SPLIT_RING - 1) % CEM_SPLIT_RING], wq.pos);     // the group RING - 1 chunks ahead (possibly the next stage's)
        wq.pos = (wq.pos + 1 == wq.n) ? 0 : wq.pos + 1;
        __builtin_amdgcn_sched_barrier(0);
        const cem_u4 (&g)[6] = wq.slot[P % CEM_SPLIT_RING];
        if (OWN && P == 0) {
            // the wave's own chunk: half of its MFMAs cover the wait at the barrier, the other half the LDS round trip of chunk 1
#pragma unroll
            for (int c = 0; c < RC; ++c) CEM_SPLIT_PRODUCTS(g, own[c][0], own[c][1], own[c][2], c, 0);
            if (XMODE == CEM_X_EXCHANGE) __syncthreads();
            if (NCH > 1) CEM_SPLIT_READ(1);
#pragma unroll
            for (int c = 0; c < RC; ++c) CEM_SPLIT_PRODUCTS(g, own[c][0], own[c][1], own[c][2], c, 1);
            continue;
        }
        if (!OWN && P == 0) {
            if (XMODE == CEM_X_EXCHANGE) __syncthreads();
            CEM_SPLIT_READ(0);
        }
        if (P + 1 < NCH && P + 1 > FL) CEM_SPLIT_READ(P + 1);       // a chunk ahead of its MFMAs
#pragma unroll
        for (int c = 0; c < RC; ++c) CEM_SPLIT_PRODUCTS(g, bp[P & 1][c][0], bp[P & 1][c][1], bp[P & 1][c][2], c, 2);
    }
#undef CEM_SPLIT_PRODUCTS
#undef CEM_SPLIT_READ
}

// The tile (cem_rollout_tile_split) is cem_rollout_chunked.h's body with three planes, split by the publishing wave:
#define CEM_CHUNKED_TILE cem_rollout_tile_split
#define CEM_CHUNKED_PLANES 3
#define CEM_CHUNKED_RING CEM_SPLIT_RING
#define CEM_CHUNKED_STAGE cem_split_stage
#define CEM_CHUNKED_OWN(OWN_, RC_) cem_u4 OWN_[RC_][3]; \
    _Pragma("unroll") for (int c = 0; c < (RC_); ++c) \
        _Pragma("unroll") for (int jj = 0; jj < 3; ++jj) OWN_[c][jj] = (cem_u4){0u, 0u, 0u, 0u}
// the scaled input block FO_ of row chunk C_ goes to LDS as three planes of 4 bf16 per lane (its half of the lane's 16 bytes)
#define CEM_CHUNKED_PUBLISH_X(SMEM_, XW_, LANE_, X_, FO_, C_) do { cem_u2 px_[3]; cem_split4((X_), px_); \
        _Pragma("unroll") for (int j_ = 0; j_ < 3; ++j_) \
            *reinterpret_cast<cem_u2 *>((SMEM_) + (XW_) + cem_split_off((C_), (FO_) >> 1, j_, LANE_) + 8 * ((FO_) & 1)) = px_[j_]; } while (0)
#define CEM_CHUNKED_PUBLISH_H(SMEM_, XW_, LANE_, W_, H0_, H1_, OWN_, C_) do { cem_split8(H0_, H1_, OWN_[C_]); \
        _Pragma("unroll") for (int j_ = 0; j_ < 3; ++j_) \
            *reinterpret_cast<cem_u4 *>((SMEM_) + (XW_) + cem_split_off(C_, W_, j_, LANE_)) = OWN_[C_][j_]; } while (0)
#include "cem_rollout_chunked.h"

template <int RC, int NFW, int MODE>
__global__ __launch_bounds__(256) void cem_rollout_split_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_tile_sample_actions(p, (int)blockIdx.x, 0, p.H, true, MODE == 1);
    cem_rollout_tile_split<RC, NFW, MODE>(p, smem, (int)blockIdx.x);
}

