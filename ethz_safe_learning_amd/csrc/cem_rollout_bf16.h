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
// Structure: the one-plane form of cem_rollout_tile_split — 4 waves per tile of 16 RC rows of one member for the whole horizon, wave w
// computes output blocks 2w, 2w + 1 of a hidden layer and keeps them, rounded, as its own K = 32 chunk of the next stage; the other
// chunks travel through LDS as ONE bf16 plane, [2 buffers][RC][4 chunks][64 lanes][16 B]; weights stream from a per-wave image of 2 KB
// groups ({a, b} output block x [64 lanes][8 bf16]) in the split kernel's visiting order (cem_split_perm).  One MFMA per (chunk, output
// block) where the split kernel issues six, one plane where it moves three, one conversion where it splits.  A stage's LDS chunks are
// all read right behind its barrier (at most 12 RC VGPRs): a chunk's MFMAs are 32 RC cycles, shorter than an LDS round trip.
// Whole-horizon tiles only (no floating segments); MODE 1 also serves cem_unfold_sequences (trajectory / head-moment outputs).
//
// A translation unit of its own (cem_rollout_bf16.hip defines CEM_ROLLOUT_BF16_UNIT): cem_capi.hip sees the launcher's declaration
// alone, so none of its kernels is compiled beside this one.
#pragma once
#include "cem_device.h"
#include "cem_rollout_split.h"

#define CEM_BF16_XB(RC_) ((RC_) * CEM_SPLIT_CHUNKS * 1024)
#define CEM_BF16_LDS_BYTES(RC_) ((size_t)2 * CEM_BF16_XB(RC_) + CEM_PART_FLOATS * 4)

// Weight ring depth: CEM_BF16_RING slots of 8 VGPRs, RING - 1 groups ahead of the MFMAs.  Every stage must be a multiple of RING chunks
// long for the slot of a chunk to be a compile-time constant, so a ring of 4 pads the two-chunk layer 0 of the obs + act <= 64 family
// with two zero-weight chunks (+11 % weight bytes and MFMAs at depth 4); 2 pads nothing.  Measured 2 vs 4, launch ms on one device
// (profiles/bf16_rollout_isa.txt): B1 0.0656 vs 0.0618, B2 0.104 vs 0.105, B3 0.702 vs 0.731, B4 0.434 vs 0.567 (16 more VGPRs cost the
// four-chunk tile of the obs + act > 64 family its second resident workgroup).
#ifndef CEM_BF16_RING
#define CEM_BF16_RING 2
#endif
__host__ __device__ constexpr int cem_bf16_l0_chunks(int nfw) { return 2 * nfw < CEM_BF16_RING ? CEM_BF16_RING : (2 * nfw + CEM_BF16_RING - 1) / CEM_BF16_RING * CEM_BF16_RING; }

// mode 0: planning; mode 1: caller-supplied noise tensors, trajectory and head-moment outputs.  Weak: a library built from cem_capi.hip
// alone (the host sanitizer build) has no bf16 rollout and says so (CEM_ERR_UNSUPPORTED at create).
__attribute__((weak)) hipError_t launch_rollout_bf16(int rc, int nfw, int mode, const RolloutParams &p, int n_tiles, hipStream_t st);

#ifdef CEM_ROLLOUT_BF16_UNIT

__device__ __forceinline__ int cem_bf16_off(const int c_rc, const int chunk, const int lane) { return ((c_rc * CEM_SPLIT_CHUNKS + chunk) * 64 + lane) * 16; }

__device__ __forceinline__ unsigned cem_bf16_pair(const float x0, const float x1)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f2){x0, x1}, cem_bf2));
}

struct BRing {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff, n, pos;
    cem_u4 slot[CEM_BF16_RING][2];
    __device__ __forceinline__ void ld(cem_u4 (&s)[2], const int g) const
    {
        s[0] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, g * 2048, 0);
        s[1] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, g * 2048 + 1024, 0);
    }
    __device__ __forceinline__ void init(const f4 *b, const int lane_, const int n_)
    {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<f4 *>(b), 0, n_ * 2048, 0x00020000);
        voff = lane_ * 16; n = n_;
#pragma unroll
        for (int i = 0; i < CEM_BF16_RING - 1; ++i) ld(slot[i], i % n_);
        pos = (CEM_BF16_RING - 1) % n_;
    }
};

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

// One tile for the whole horizon (cem_rollout_tile_split with one plane; MODE as there)
template <int RC, int NFW, int MODE>
__device__ __forceinline__ void cem_rollout_tile_bf16(const RolloutParams &p, char *smem, const int tile_idx)
{
    const int tid = (int)((threadIdx.x + 64u * (unsigned)((tile_idx + (tile_idx >> 8)) & 3)) & 255u);   // wave roles rotate with the tile
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int j = lane & 15, q = lane >> 4;
    const TileDesc td = p.tiles[tile_idx];
    const int wbk = 0;
    const int O = p.O, A = p.A, H = p.H;
    constexpr int XB = CEM_BF16_XB(RC);
    constexpr int NCH0 = cem_bf16_l0_chunks(NFW);         // K = 32 chunks of the layer-0 input (padded to the ring length)
    float *part = reinterpret_cast<float *>(smem + 2 * XB);
    int xw = 0;
    if (NCH0 > 2 * NFW) {                                 // padded layer-0 chunks meet zero weights: what LDS holds there must be finite
        for (int o = (int)threadIdx.x * 16; o < 2 * XB; o += 256 * 16) *reinterpret_cast<cem_u4 *>(smem + o) = (cem_u4){0u, 0u, 0u, 0u};
        __syncthreads();
    }
    const PhiloxKey key = cem_key(p.ctrl);
    const float rscale = p.sampling ? CEM_BM_RSCALE : 0.0f;
    const int member_u = __builtin_amdgcn_readfirstlane(td.member);
    BRing wq;
    wq.init(p.wpack + (size_t)member_u * p.member_stride_f4 + p.wave_off_f4[w], lane, (int)p.wave_groups[w]);
    const __amdgpu_buffer_rsrc_t et_rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.etab + (size_t)member_u * (CEM_ET_ROWS + p.L) * CEM_U), 0, (CEM_ET_ROWS + p.L) * CEM_U * 4, 0x00020000);
    const int tab_v = 64 * w + 16 * q;
    const int bias_v = 128 * w + 16 * q;

    f4 s[NFW][RC];
    int slotc[RC];
#pragma unroll
    for (int c = 0; c < RC; ++c) { const int sl = 16 * c + j; slotc[c] = sl < td.cnt ? sl : td.cnt - 1; }
#pragma unroll
    for (int i = 0; i < NFW; ++i) {
        const int f0 = 16 * (w + 4 * i) + 4 * q;
#pragma unroll
        for (int c = 0; c < RC; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = f0 + r;
                float v = 0.f;
                if (f < O) v = td.s0_base < 0 ? p.ctrl->state[f] : p.s0[(size_t)(td.s0_base + slotc[c]) * O + f];
                s[i][c][r] = v;
            }
    }
    const __amdgpu_buffer_rsrc_t act_rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<f4 *>(p.act_pad), 0, MODE == 0 ? p.act_pad_bytes : 0u, 0x00020000);
    int actv[NFW][RC];
    const float *actrow[RC];
#pragma unroll
    for (int c = 0; c < RC; ++c) {
        actrow[c] = p.actions + (size_t)(td.act_base + slotc[c]) * H * A;
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            int qi = 4 * (w + 4 * i) + q - p.act_q0;
            qi = qi < 0 ? 0 : (qi >= p.act_nq ? p.act_nq - 1 : qi);
            actv[i][c] = ((td.act_base + slotc[c]) * H * p.act_nq + qi) * 16;
        }
    }
    // the scaled input block Fo of chunk c_rc goes to LDS rounded: 4 bf16 per lane (its half of the lane's 16 bytes)
#define CEM_PUBLISH_X(X_, FO_, C_) do { \
        *reinterpret_cast<cem_u2 *>(smem + xw + cem_bf16_off((C_), (FO_) >> 1, lane) + 8 * ((FO_) & 1)) = \
            (cem_u2){cem_bf16_pair((X_)[0], (X_)[1]), cem_bf16_pair((X_)[2], (X_)[3])}; } while (0)

    float d_prev = 0.f, c_prev = 0.f, cum = 0.f;
    bool done = false;
    const int nk = 1 + p.sc.n_cost;
    const float csz[4] = {p.sc.cost_size[0], p.sc.cost_size[1], p.sc.cost_size[2], p.sc.cost_size[3]};
    const float ind_cap = p.sc.indicator ? 1.0f : __builtin_inff(), clipv = p.sc.reward_clip > 0.f ? p.sc.reward_clip : __builtin_inff();
    const __amdgpu_buffer_rsrc_t cost_rs = __builtin_amdgcn_make_buffer_rsrc(p.costs, 0, p.costs ? (uint32_t)(H * p.Bloc) : 0u, 0x00020000);

    // ---- prologue: x_0 = scale(concat[s_0, a_0]) and the scorer terms of s_0 --------------------------------------------------
    {
        float pm[2][RC];
#pragma unroll
        for (int c = 0; c < RC; ++c) { pm[0][c] = __builtin_inff(); pm[1][c] = __builtin_inff(); }
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            const int tv = tab_v + 256 * i;
            const f4 mn4 = cem_ld_tab(et_rs, tv, CEM_ET_NMIN * 512), rd4 = cem_ld_tab(et_rs, tv, CEM_ET_RDELTA * 512);
            const f4 isact4 = cem_ld_tab(et_rs, tv, CEM_ET_ACT * 512);
            const f4 sel0 = cem_ld_tab(et_rs, tv, CEM_ET_SEL0 * 512), sel1 = cem_ld_tab(et_rs, tv, CEM_ET_SEL1 * 512);
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                f4 act4; CEM_LOAD_ACT(act4, MODE, p, act_rs, actv, actrow, w, q, O, A, i, c, 0);
                const f4 sn = s[i][c];
                if (MODE == 1) {
                    const int slot = 16 * c + j, f0 = 16 * (w + 4 * i) + 4 * q;
                    if (p.traj && slot < td.cnt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (f0 + r < O) p.traj[((size_t)(td.row_base + slot) * (H + 1)) * O + f0 + r] = sn[r];
                    }
                }
                cem_scorer_terms(sn, p.sc.D, sel0, sel1, pm[0][c], pm[1][c]);
                const f4 x = cem_sub4(__builtin_elementwise_fma(isact4, act4, sn), mn4) * rd4;
                CEM_PUBLISH_X(x, w + 4 * i, c);
            }
        }
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_MEM, et_rs);
        xw = XB;
    }
    f4 nb0 = cem_ld_tab(et_rs, bias_v, CEM_ET_ROWS * 512);
    f4 nb1 = cem_ld_tab(et_rs, bias_v + 64, CEM_ET_ROWS * 512);
    cem_u4 own[RC];                                       // the wave's own chunk (its two output blocks of the last hidden stage), rounded
#pragma unroll
    for (int c = 0; c < RC; ++c) own[c] = (cem_u4){0u, 0u, 0u, 0u};

    const int prio_r0 = (tile_idx >> 8) % 3;
    f4 bm0, bv0;
    for (int t = 0; t < H; ++t) {
        {
            const int lvl = (t + prio_r0) % 3;
            if (lvl == 0) __builtin_amdgcn_s_setprio(0); else if (lvl == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2);
        }
        // relu, round, keep as the own chunk and publish: 4 v_cvt_pk_bf16_f32 per 8 activations
#define CEM_BF16_PUBLISH() do { \
            _Pragma("unroll") for (int c = 0; c < RC; ++c) { \
                f4 h0 = acc0[c], h1 = acc1[c]; \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) { h0[r] = fmaxf(h0[r], 0.f); h1[r] = fmaxf(h1[r], 0.f); } \
                own[c] = (cem_u4){cem_bf16_pair(h0[0], h0[1]), cem_bf16_pair(h0[2], h0[3]), cem_bf16_pair(h1[0], h1[1]), cem_bf16_pair(h1[2], h1[3])}; \
                *reinterpret_cast<cem_u4 *>(smem + xw + cem_bf16_off(c, w, lane)) = own[c]; \
            } \
            xw ^= XB; } while (0)
#define CEM_NEXT_BIAS(LN) do { \
            nb0 = cem_ld_tab(et_rs, bias_v, (CEM_ET_ROWS + (LN)) * 512); \
            nb1 = cem_ld_tab(et_rs, bias_v + 64, (CEM_ET_ROWS + (LN)) * 512); } while (0)
        {
            f4 acc0[RC], acc1[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c) { acc0[c] = nb0; acc1[c] = nb1; }
            CEM_NEXT_BIAS(p.L > 1 ? 1 : 0);
            // layer 0: every chunk of the scaled input comes from LDS (a wave's input blocks w, w + 4 are halves of two chunks)
            cem_bf16_stage<RC, NCH0, false, CEM_X_EXCHANGE>(acc0, acc1, own, wq, smem, xw ^ XB, lane, w);
            // the head biases of the wave's first observation block, requested a step's worth of hidden stages ahead of their use
            bm0 = cem_ld_tab(et_rs, tab_v, CEM_ET_BMU * 512); bv0 = cem_ld_tab(et_rs, tab_v, CEM_ET_BVAR * 512);
            CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, t - 1);
            CEM_BF16_PUBLISH();
        }
        for (int l = 1; l < p.L; ++l) {
            f4 acc0[RC], acc1[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c) { acc0[c] = nb0; acc1[c] = nb1; }
            CEM_NEXT_BIAS(l + 1 < p.L ? l + 1 : 0);
            cem_bf16_stage<RC, CEM_SPLIT_CHUNKS, true, CEM_X_EXCHANGE>(acc0, acc1, own, wq, smem, xw ^ XB, lane, w);
            CEM_BF16_PUBLISH();
        }
#undef CEM_BF16_PUBLISH
#undef CEM_NEXT_BIAS

        // ---- heads, state update, scorer terms, next scaled input: cem_rollout_tile's epilogue ------------------------------------
        float pm[2][RC];
#pragma unroll
        for (int c = 0; c < RC; ++c) { pm[0][c] = __builtin_inff(); pm[1][c] = __builtin_inff(); }
        const int tn = (t + 1 < H) ? t + 1 : H - 1;
#pragma unroll
        for (int i = 0; i < NFW; ++i) {
            const int Fo = w + 4 * i;
            const int tv = tab_v + 256 * i;
            const f4 mn4 = cem_ld_tab(et_rs, tv, CEM_ET_NMIN * 512), rd4 = cem_ld_tab(et_rs, tv, CEM_ET_RDELTA * 512);
            const f4 bm = i == 0 ? bm0 : cem_ld_tab(et_rs, tv, CEM_ET_BMU * 512), bv = i == 0 ? bv0 : cem_ld_tab(et_rs, tv, CEM_ET_BVAR * 512);
            const f4 om4 = cem_ld_tab(et_rs, tv, CEM_ET_OBS * 512), isact4 = cem_ld_tab(et_rs, tv, CEM_ET_ACT * 512);
            const f4 sel0 = cem_ld_tab(et_rs, tv, CEM_ET_SEL0 * 512), sel1 = cem_ld_tab(et_rs, tv, CEM_ET_SEL1 * 512);
            f4 accm[RC], accv[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c) { accm[c] = bm; accv[c] = bv; }
            if (Fo < p.KB_obs) {                                                           // wave-uniform
                if (i == 0) cem_bf16_stage<RC, CEM_SPLIT_CHUNKS, true, CEM_X_EXCHANGE>(accm, accv, own, wq, smem, xw ^ XB, lane, w);
                else cem_bf16_stage<RC, CEM_SPLIT_CHUNKS, true, CEM_X_REREAD>(accm, accv, own, wq, smem, xw ^ XB, lane, w);
            } else if (i == 0) {
                __syncthreads();                      // keep the barrier count of waves without observation features
            }
            // the step's model noise and actions: independent of the heads' MFMAs, so drawn after they are issued
            f4 act4[RC], eps4[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                CEM_LOAD_ACT(act4[c], MODE, p, act_rs, actv, actrow, w, q, O, A, i, c, tn);
                CEM_MODEL_NOISE4(eps4[c], MODE, p, td, 0, O, t, t, slotc[c], Fo, q, key, rscale);
            }
#pragma unroll
            for (int c = 0; c < RC; ++c) {
                const f4 mu = accm[c];
                const f4 var = cem_softplus4(accv[c]) + 1e-4f;
                f4 sd;
#pragma unroll
                for (int r = 0; r < 4; ++r) sd[r] = __builtin_amdgcn_sqrtf(var[r]);
                const f4 d = mu + sd * eps4[c];
                const f4 sn = s[i][c] + d * om4;
                if (MODE == 1) {
                    const int slot = 16 * c + j, f0 = 16 * Fo + 4 * q;
                    if (slot < td.cnt) {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                            if (f0 + r < O) {
                                const size_t o = ((size_t)(td.row_base + slot) * H + t) * O + f0 + r;
                                if (p.mu_out) p.mu_out[o] = mu[r];
                                if (p.sd_out) p.sd_out[o] = sd[r];
                                if (p.traj) p.traj[((size_t)(td.row_base + slot) * (H + 1) + (t + 1)) * O + f0 + r] = sn[r];
                            }
                    }
                }
                s[i][c] = sn;
                cem_scorer_terms(sn, p.sc.D, sel0, sel1, pm[0][c], pm[1][c]);
                const f4 x = cem_sub4(__builtin_elementwise_fma(isact4, act4[c], sn), mn4) * rd4;
                CEM_PUBLISH_X(x, Fo, c);
            }
        }
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_MEM, et_rs);
        xw ^= XB;
    }
    __syncthreads();
    CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, H - 1);
    if (w == wbk && lane < td.cnt) p.ret[td.row_base + lane] = cum;
#undef CEM_PUBLISH_X
}

template <int RC, int NFW, int MODE>
__global__ __launch_bounds__(256) void cem_rollout_bf16_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_tile_sample_actions(p, (int)blockIdx.x, 0, p.H, true, MODE == 1);
    cem_rollout_tile_bf16<RC, NFW, MODE>(p, smem, (int)blockIdx.x);
}

#endif  // CEM_ROLLOUT_BF16_UNIT
