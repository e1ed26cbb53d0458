// cem_rollout_chunked.h — the whole-horizon tile of the "chunked" rollouts, written ONCE: cem_rollout_split_kernel (cem_rollout_split.h,
// three bf16 planes) and cem_rollout_bf16_kernel (cem_rollout_bf16.h, one) run a dense stage as K = 32 chunks on the bf16 matrix pipe,
// wave w keeping output blocks 2w, 2w + 1 of a hidden stage as its own chunk of the next, the other chunks travelling through LDS.
// All around the stages is the same code: tile set-up, state load, action offsets, prologue, step loop, layer 0 / hidden / heads, the
// barrier-count rule of waves without observation blocks, epilogue, bookkeeping (cem_rollout_common.h's pieces, arguments explicit).
//
// A body to be INCLUDED once per variant (no include guard around it; like cem_tile_costs.inc): the including header defines the
// variant's hooks, includes this file and gets CEM_CHUNKED_TILE<RC, NFW, MODE>(params, smem, tile); the hooks are undefined again at
// the end.  Every name a hook touches is an argument:
//   CEM_CHUNKED_TILE                       the tile function to define (cem_rollout_tile_split, cem_rollout_tile_bf16)
//   CEM_CHUNKED_PLANES, CEM_CHUNKED_RING   bf16 planes an activation travels as; depth of the weight ring (ChunkRing, cem_rollout_split.h)
//   CEM_CHUNKED_OWN(OWN_, RC_)             declares the wave's own K = 32 chunk of every row chunk, in registers, all zero
//   CEM_CHUNKED_PUBLISH_X(SMEM_, XW_, LANE_, X_, FO_, C_)              the scaled layer-0 input block FO_ of row chunk C_ -> LDS
//   CEM_CHUNKED_PUBLISH_H(SMEM_, XW_, LANE_, W_, H0_, H1_, OWN_, C_)   row chunk C_'s post-ReLU accumulator quads -> OWN_[C_] -> LDS, chunk W_
//   CEM_CHUNKED_STAGE                      the stage function template, <RC, NCH, OWN, XMODE>(acc0, acc1, own, ring, smem, xr, lane, w)
// Why a textual body and not a function template over a traits struct: profiles/chunked_rollout_isa.txt (the forms tried, the registers moved).

#ifndef CEM_ROLLOUT_CHUNKED_ONCE
#define CEM_ROLLOUT_CHUNKED_ONCE
#define CEM_CHUNKED_XB(PLANES_, RC_) ((RC_) * CEM_SPLIT_CHUNKS * (PLANES_) * 1024)          // LDS bytes of one activation buffer
#define CEM_CHUNKED_LDS_BYTES(PLANES_, RC_) ((size_t)2 * CEM_CHUNKED_XB(PLANES_, RC_) + CEM_PART_FLOATS * 4)
// K = 32 chunks of the layer-0 input of the NFW family, padded to a multiple of the ring depth so that every stage keeps the ring
// phase (the padding meets zero weights; at depth 2 there is none: 2 * nfw).  Host (stream lengths, packers) and device.
__host__ __device__ constexpr int cem_chunked_l0_chunks(int nfw, int ring) { return 2 * nfw < ring ? ring : (2 * nfw + ring - 1) / ring * ring; }

// The launcher of a variant's kernels, NAME_(rc, nfw, mode, params, n_tiles, stream): mode 0 planning, mode 1 caller-supplied noise
// tensors with trajectory / head-moment outputs.  One dispatch for both variants; expanded in the translation unit that holds KERNEL_.
#define CEM_CHUNKED_LAUNCH_CASE(KERNEL_, PLANES_, R_, F_) \
    if (rc == R_ && nfw == F_) { \
        if (mode) hipLaunchKernelGGL((KERNEL_<R_, F_, 1>), dim3(n_tiles), dim3(256), CEM_CHUNKED_LDS_BYTES(PLANES_, R_), st, p); \
        else hipLaunchKernelGGL((KERNEL_<R_, F_, 0>), dim3(n_tiles), dim3(256), CEM_CHUNKED_LDS_BYTES(PLANES_, R_), st, p); \
        return hipGetLastError(); }
#define CEM_CHUNKED_LAUNCH_ROW(K_, PL_, F_) CEM_CHUNKED_LAUNCH_CASE(K_, PL_, 1, F_) CEM_CHUNKED_LAUNCH_CASE(K_, PL_, 2, F_) CEM_CHUNKED_LAUNCH_CASE(K_, PL_, 3, F_) CEM_CHUNKED_LAUNCH_CASE(K_, PL_, 4, F_)
#define CEM_CHUNKED_LAUNCHER(NAME_, KERNEL_, PLANES_) \
    hipError_t NAME_(int rc, int nfw, int mode, const RolloutParams &p, int n_tiles, hipStream_t st) \
    { \
        if ((mode != 0 && mode != 1) || n_tiles < 1) return hipErrorInvalidValue; \
        CEM_CHUNKED_LAUNCH_ROW(KERNEL_, PLANES_, 1) CEM_CHUNKED_LAUNCH_ROW(KERNEL_, PLANES_, 2) \
        return hipErrorInvalidValue; \
    }
#endif  // CEM_ROLLOUT_CHUNKED_ONCE

// One tile for the whole horizon (cem_rollout_tile with the variant's stages; MODE as there)
template <int RC, int NFW, int MODE>
__device__ __forceinline__ void CEM_CHUNKED_TILE(const RolloutParams &p, char *smem, const int tile_idx)
{
    const int tid = (int)((threadIdx.x + 64u * (unsigned)((tile_idx + (tile_idx >> 8)) & 3)) & 255u);   // wave roles rotate with the tile
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int j = lane & 15, q = lane >> 4;
    const TileDesc td = p.tiles[tile_idx];
    const int wbk = 0;
    const int O = p.O, A = p.A, H = p.H;
    constexpr int XB = CEM_CHUNKED_XB(CEM_CHUNKED_PLANES, RC);
    constexpr int NCH0 = cem_chunked_l0_chunks(NFW, CEM_CHUNKED_RING);   // K = 32 chunks of the layer-0 input (padded to the ring length)
    float *part = reinterpret_cast<float *>(smem + 2 * XB);
    int xw = 0;
    if (NCH0 > 2 * NFW) {                                 // padded layer-0 chunks meet zero weights: what LDS holds there must be finite
        for (int o = (int)threadIdx.x * 16; o < 2 * XB; o += 256 * 16) *reinterpret_cast<cem_u4 *>(smem + o) = (cem_u4){0u, 0u, 0u, 0u};
        __syncthreads();
    }
    const PhiloxKey key = cem_key(p.ctrl);
    const float rscale = p.sampling ? CEM_BM_RSCALE : 0.0f;
    const int member_u = __builtin_amdgcn_readfirstlane(td.member);
    ChunkRing<2 * CEM_CHUNKED_PLANES, CEM_CHUNKED_RING> wq;
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
                CEM_CHUNKED_PUBLISH_X(smem, xw, lane, x, w + 4 * i, c);
            }
        }
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_MEM, et_rs);
        xw = XB;
    }
    f4 nb0 = cem_ld_tab(et_rs, bias_v, CEM_ET_ROWS * 512);
    f4 nb1 = cem_ld_tab(et_rs, bias_v + 64, CEM_ET_ROWS * 512);
    CEM_CHUNKED_OWN(own, RC);                             // the wave's own chunk (its two output blocks of the last hidden stage), all zero

#ifdef CEM_STAMPS
    long long st_[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    long long tprev_ = (long long)__builtin_amdgcn_s_memtime();
    st_[7] = tprev_;
#endif
    const int prio_r0 = (tile_idx >> 8) % 3;
    f4 bm0, bv0;
    for (int t = 0; t < H; ++t) {
        {
            const int lvl = (t + prio_r0) % 3;
            if (lvl == 0) __builtin_amdgcn_s_setprio(0); else if (lvl == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2);
        }
        // relu, keep as the own chunk and publish
#define CEM_CHUNKED_PUBLISH() do { \
            _Pragma("unroll") for (int c = 0; c < RC; ++c) { \
                f4 h0 = acc0[c], h1 = acc1[c]; \
                _Pragma("unroll") for (int r = 0; r < 4; ++r) { h0[r] = fmaxf(h0[r], 0.f); h1[r] = fmaxf(h1[r], 0.f); } \
                CEM_CHUNKED_PUBLISH_H(smem, xw, lane, w, h0, h1, own, c); \
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
            CEM_CHUNKED_STAGE<RC, NCH0, false, CEM_X_EXCHANGE>(acc0, acc1, own, wq, smem, xw ^ XB, lane, w);
            // the head biases of the wave's first observation block start the heads' accumulators: requested here, a step's worth of
            // hidden stages ahead (requested next to their use they cost the heads stage an L2 round trip: 2.26 K vs 1.8 K cycles)
            bm0 = cem_ld_tab(et_rs, tab_v, CEM_ET_BMU * 512); bv0 = cem_ld_tab(et_rs, tab_v, CEM_ET_BVAR * 512);
            CEM_STAMP(0);
            CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, t - 1);
            CEM_STAMP(6);
            CEM_CHUNKED_PUBLISH();
            CEM_STAMP(5);
        }
        for (int l = 1; l < p.L; ++l) {
            f4 acc0[RC], acc1[RC];
#pragma unroll
            for (int c = 0; c < RC; ++c) { acc0[c] = nb0; acc1[c] = nb1; }
            CEM_NEXT_BIAS(l + 1 < p.L ? l + 1 : 0);
            CEM_CHUNKED_STAGE<RC, CEM_SPLIT_CHUNKS, true, CEM_X_EXCHANGE>(acc0, acc1, own, wq, smem, xw ^ XB, lane, w);
            CEM_STAMP(1);
            CEM_CHUNKED_PUBLISH();
            CEM_STAMP(5);
        }
#undef CEM_CHUNKED_PUBLISH
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
            CEM_STAMP(2);
            if (Fo < p.KB_obs) {                                                           // wave-uniform
                if (i == 0) CEM_CHUNKED_STAGE<RC, CEM_SPLIT_CHUNKS, true, CEM_X_EXCHANGE>(accm, accv, own, wq, smem, xw ^ XB, lane, w);
                else CEM_CHUNKED_STAGE<RC, CEM_SPLIT_CHUNKS, true, CEM_X_REREAD>(accm, accv, own, wq, smem, xw ^ XB, lane, w);
            } else if (i == 0) {
                __syncthreads();                      // keep the barrier count of waves without observation features
            }
            CEM_STAMP(3);
            // the step's model noise and actions: independent of the heads' MFMAs, so drawn AFTER they are issued — VALU work behind
            // queued bf16 MFMAs runs in their shadow (scripts/mfma_microbench5.hip -DMB_BF16: 288 MFMAs + 330 VALU take 1.08 x the MFMAs alone)
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
                CEM_CHUNKED_PUBLISH_X(smem, xw, lane, x, Fo, c);
            }
        }
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_MEM, et_rs);
        xw ^= XB;
        CEM_STAMP(4);
    }
    __syncthreads();
    CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, H - 1);
    if (w == wbk && lane < td.cnt) p.ret[td.row_base + lane] = cum;
#ifdef CEM_STAMPS
    if (p.stamps && lane == 0) for (int i = 0; i < 8; ++i) p.stamps[((size_t)tile_idx * 4 + w) * 8 + i] = st_[i];
#endif
}

#undef CEM_CHUNKED_TILE
#undef CEM_CHUNKED_PLANES
#undef CEM_CHUNKED_RING
#undef CEM_CHUNKED_OWN
#undef CEM_CHUNKED_PUBLISH_X
#undef CEM_CHUNKED_PUBLISH_H
#undef CEM_CHUNKED_STAGE
