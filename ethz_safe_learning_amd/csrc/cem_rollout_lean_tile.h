// cem_rollout_lean_tile.h — the tile of the lean one-chunk rollout, written ONCE for its two forms: the branchy one (cem_rollout_lean.hip,
// the bit-exact reference and the fallback) and the straight-line one (cem_rollout_lean_straight.hip).  Both are cem_rollout_tile<1, 1, 0,
// SEG> — the weight ring, stage order, barriers per step, bookkeeping and hand-over are that function's; the comments there apply — with
// the lean path's own set-up and epilogue, which is all here: the lane and role preamble, the table and mu / sigma / bounds fill of LDS,
// the s_0 load, the Philox counter words, the action and its parking, the resumed-segment load and the first-step block, the LDS
// addresses of the activation exchange, the step's dense layers and heads epilogue, the copy-out and the hand-over stores.
//
// A body to be INCLUDED once by each unit (no include guard; like cem_rollout_chunked.h), behind cem_rollout_lean.h and the unit's ring
// and stage.  Why textual and not one template: profiles/lean_tile_isa.txt (the forms tried, the registers they moved).  The unit defines
// the hooks below; they are expanded inside the tile and see its locals, by the names this file gives them:
//   CEM_LEAN_TILE_TEMPLATE, CEM_LEAN_TILE   the template head (its first parameter is bool SEG) and the name of the tile function
//   CEM_LEAN_HANDOVER_DECL, CEM_LEAN_HANDOVER  what the form keeps of the hand-over buffer across the step loop (from CEM_LEAN_SEG_RSRC
//                                           below) and of the bookkeeping wave's number; the buffer's descriptor at a use
//   CEM_LEAN_BKWAVE                         whether this wave keeps the books: a flag set once, or a comparison at every use
//   CEM_LEAN_RING                           declares and fills wq, the wave's weight ring (the straight-line form also its `heads`)
//   CEM_LEAN_STAGE(KF, NOWN, L0IN, BASE)    the stage function: KF groups, the first NOWN the wave's own, BASE groups of the step before it
//   CEM_LEAN_BOOKS_DECL, CEM_LEAN_SCORE_D   the scorer's scalars and the bookkeeper (d_prev, c_prev, cum, done are the tile's); sc.D
//   CEM_LEAN_STORE_TERMS                    publishes pm[2][1], the step's partial minima of the scorer terms (s: the state registers)
//   CEM_LEAN_PRIO_DECL, CEM_LEAN_PRIO_STEP  the issue-priority rotation: its state in front of the loop, the step's switch (t: the step)
//   CEM_LEAN_BOOKS_STEP, CEM_LEAN_BOOKS_END settle step t - 1 behind layer 0 of step t (first: the tile's or segment's first), and t_end - 1
//   CEM_LEAN_HIDDEN_LAYERS                  the three hidden layers, each CEM_LEAN_HIDDEN(next bias row, BASE)
//   CEM_LEAN_HEADS                          whether this wave has observation blocks of the heads stage (else it only keeps the barrier count)
//   CEM_LEAN_ISACT, CEM_LEAN_NEXT_INPUT     the epilogue's read of the action mask and the next layer-0 input from sn, e4, mn4, rd4
// All are undefined again at the end.

// the descriptor of the tile's hand-over buffer (a plain launch has none: any valid base)
#define CEM_LEAN_SEG_RSRC() __builtin_amdgcn_make_buffer_rsrc( \
        SEG ? const_cast<f4 *>(p.seg_state + (size_t)(tile_idx - p.n_pinned) * (2 * 256 + 64)) : const_cast<f4 *>(p.wpack), 0, (2 * 256 + 64) * 16, 0x00020000)
CEM_LEAN_TILE_TEMPLATE
__device__ __forceinline__ void CEM_LEAN_TILE(const RolloutParams &p, char *smem, const int tile_idx, const int t_begin, const int t_end)
{
    constexpr int RC = 1, NFW = 1;
    const int tid = (int)((threadIdx.x + 64u * (unsigned)((tile_idx + (tile_idx >> 8)) & 3)) & 255u);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int j = lane & 15, q = lane >> 4;
    const TileDesc td = p.tiles[tile_idx];
    const bool resumed = SEG && t_begin > 0;
    CEM_LEAN_HANDOVER_DECL
    const int O = p.O, A = p.A, H = p.H, AZ = (A + 3) >> 2;
    constexpr int XB = CEM_NG * 1024;
    float *part = reinterpret_cast<float *>(smem + 2 * XB);
    const CtrlBlock *const ctrl = p.ctrl;
    const PhiloxKey key = cem_key(ctrl);
    const float rscale = p.sampling ? CEM_BM_RSCALE : 0.0f;

    const int member_u = __builtin_amdgcn_readfirstlane(td.member);
    CEM_LEAN_RING

    const __amdgpu_buffer_rsrc_t et_rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.etab + (size_t)member_u * (CEM_ET_ROWS + p.L) * CEM_U), 0, (CEM_ET_ROWS + p.L) * CEM_U * 4, 0x00020000);
    const int tab_v = 64 * w + 16 * q;
    const int bias_v = 128 * w + 16 * q;
    const char *tabl = smem + 2 * XB + CEM_PART_FLOATS * 4;
    // behind the feature tables: sigma / mu of every step and the bounds, as the zero-padded quads the action lanes read in the epilogue
    // (quad z of step t at (t AZ + z) * 32: sigma, then mu; the bounds of quad z at (H AZ + z) * 32: lb, then ub)
    const char *actl = tabl + CEM_TAB_LDS_BYTES;
    {
        const int ht = (int)threadIdx.x;
        *reinterpret_cast<f4 *>(const_cast<char *>(tabl) + ht * 16) = cem_ld_tab(et_rs, (ht & 31) * 16, (ht >> 5) * 512);
        const int HA = H * A;
        for (int idx = ht; idx < (H + 1) * AZ; idx += 256) {
            const int t = idx / AZ, z = idx - t * AZ;
            const float *lo = t < H ? p.musig + HA + t * A : p.act_bounds, *hi = t < H ? p.musig + t * A : p.act_bounds + 32;
            f4 u = {0.f, 0.f, 0.f, 0.f}, v = u;
#pragma unroll
            for (int r = 0; r < 4; ++r) if (4 * z + r < A) { u[r] = lo[4 * z + r]; v[r] = hi[4 * z + r]; }
            *reinterpret_cast<f4 *>(const_cast<char *>(actl) + idx * 32) = u;
            *reinterpret_cast<f4 *>(const_cast<char *>(actl) + idx * 32 + 16) = v;
        }
    }
    __syncthreads();

    f4 s[NFW][RC];
    const int slot0 = j < td.cnt ? j : td.cnt - 1;
    {
        const int f0 = 16 * w + 4 * q;
        if (resumed) s[0][0] = cem_ld_coherent(CEM_LEAN_HANDOVER, tid * 16);
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = f0 + r;
                float v = 0.f;
                if (f < O) v = td.s0_base < 0 ? ctrl->state[f] : p.s0[(size_t)(td.s0_base + slot0) * O + f];
                s[0][0][r] = v;
            }
        }
    }

    // This lane's Philox counter words.  Action lanes (feature quad 4 w + q = O / 4 + z, 0 <= z < AZ): the action noise of (candidate,
    // step t + 1, quad z); every other lane: the model noise of (row, step t, feature quad).  Per step: one add (pc1 + t).
    const int zq = 4 * w + q - (O >> 2);
    const bool actlane = zq >= 0 && zq < AZ;
    // whether this WAVE holds an action quad at all (wave-uniform; obs 60: the wave that plays w = 3): the other waves skip the action
    // part of the epilogue outright — their isact rows are 0, and fma(0, finite, s) = s
    const bool wact = 4 * w + 3 >= (O >> 2) && 4 * w < (O >> 2) + AZ;
    const int zc = actlane ? zq : 0;
    const uint32_t pc0 = (uint32_t)((actlane ? td.act_base : td.noise_row_base) + slot0);
    const uint32_t pc2 = actlane ? ((uint32_t)zc | (CEM_STREAM_ACT << 16)) : ((uint32_t)(4 * w + q) | (CEM_STREAM_MODEL << 16));
    const uint32_t pc1 = ((uint32_t)p.it << 16) + (actlane ? 1u : 0u);
    const float prs = actlane ? CEM_BM_RSCALE : rscale;          // sampling_propagation False zeroes the model noise only
    const char *const actl_v = actl + zc * 32;
    // cem_mpc.py:44-48 on this lane's quad: eps * sigma + mu as a separate multiply and add (tf.random.normal), then tf.clip_by_value;
    // the moments and bounds come out of LDS at the point of use
#define CEM_LEAN_ACTION(DST, E_, T_) do { \
        const char *m_ = actl_v + (T_) * AZ * 32, *b_ = actl_v + H * AZ * 32; \
        const f4 sg_ = *reinterpret_cast<const f4 *>(m_), mu_ = *reinterpret_cast<const f4 *>(m_ + 16); \
        const f4 lb_ = *reinterpret_cast<const f4 *>(b_), ub_ = *reinterpret_cast<const f4 *>(b_ + 16); \
        f4 v_ = (E_) * sg_; v_ = v_ + mu_; \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) DST[r] = fminf(fmaxf(v_[r], lb_[r]), ub_[r]); } while (0)
    // The select and cem_planner_actions read the natural [N][H][A] array, which the tiles of particle 0 write.  Not step by step: a
    // store in the step loop sits in the same vmcnt queue as the weight ring, and every wait for a weight group behind it would wait
    // for the store's acknowledgement too.  The action lanes of valid rows park their quads in LDS ([row][H + 1][AZ] quads; step H is
    // the scratch slot of the last step's unused draw, row 16 that of the lanes that keep nothing) and the workgroup copies them out
    // once, behind the last step.
    const bool act_keep = actlane && j < td.cnt && td.row_base < p.Nloc;
    char *const stage = const_cast<char *>(actl) + (H + 1) * AZ * 32;
    char *const stage_v = stage + ((act_keep ? j : 16) * (H + 1) * AZ + zc) * 16;
#define CEM_LEAN_KEEP(V_, T_) do { *reinterpret_cast<f4 *>(stage_v + (T_) * AZ * 16) = (V_); } while (0)

    float d_prev = 0.f, c_prev = 0.f, cum = 0.f;
    bool done = false;
    CEM_LEAN_BOOKS_DECL

    f4 hB[CEM_NG][RC];
    if (resumed) {
        // (the hand-over carries the next layer-0 input, the action of step t_begin inside it: nothing is drawn again)
        const __amdgpu_buffer_rsrc_t ho = CEM_LEAN_HANDOVER;
        const f4 x = cem_ld_coherent(ho, (256 + tid) * 16);
        hB[0][0] = x;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        if (CEM_LEAN_BKWAVE) {
            const f4 b = cem_ld_coherent(ho, (2 * 256 + lane) * 16);
            d_prev = b[0]; c_prev = b[1]; cum = b[2]; done = b[3] != 0.f;
        }
    } else {
        float pm[2][RC];
        pm[0][0] = __builtin_inff(); pm[1][0] = __builtin_inff();
        const int tv = tab_v;
        const f4 mn4 = CEM_TAB(tabl, CEM_ET_NMIN, tv), rd4 = CEM_TAB(tabl, CEM_ET_RDELTA, tv);
        const f4 isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv);
        const f4 sel0 = CEM_TAB(tabl, CEM_ET_SEL0, tv), sel1 = CEM_TAB(tabl, CEM_ET_SEL1, tv);
        // the action of step 0: the tile's one extra draw
        const f4 e0 = cem_normal4(pc0, 0u, (uint32_t)p.it, (uint32_t)zc, CEM_STREAM_ACT, key);
        const f4 sn = s[0][0];
        f4 xin = sn;
        if (wact) {
            f4 act4; CEM_LEAN_ACTION(act4, e0, 0);
            CEM_LEAN_KEEP(act4, 0);
            xin = __builtin_elementwise_fma(isact4, act4, sn);
        }
        cem_scorer_terms(sn, CEM_LEAN_SCORE_D, sel0, sel1, pm[0][0], pm[1][0]);
        const f4 x = cem_sub4(xin, mn4) * rd4;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        hB[0][0] = x;
        CEM_LEAN_STORE_TERMS;
    }
    f4 nb0 = cem_ld_tab(et_rs, bias_v, CEM_ET_ROWS * 512);
    f4 nb1 = cem_ld_tab(et_rs, bias_v + 64, CEM_ET_ROWS * 512);

    // LDS addresses of the stages' reads and writes, less the exchange buffer: the other waves' blocks of a hidden / heads stage
    // (cem_perm_hidden: ascending, own blocks 2w, 2w + 1 skipped) and of layer 0 (cem_perm_l0: own block w skipped), this wave's
    // output blocks and its layer-0 input block
    const char *rbh[6], *rb0[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) rbh[k] = smem + lane * 16 + (k < 2 * w ? 0 : 2048);
#pragma unroll
    for (int k = 0; k < 3; ++k) rb0[k] = smem + lane * 16 + (k < w ? 0 : 1024);
    char *const pubh = smem + (2 * w * 64 + lane) * 16, *const pub0 = smem + (w * 64 + lane) * 16;
    CEM_LEAN_PRIO_DECL
    // The exchange buffer toggles five times a step (depth 4: layer 0, three hidden layers, the heads; lean_eligible), so its parity
    // alternates with the step: the loop runs two steps per round, each with the buffer offsets as compile-time constants, and leaves
    // between them when the count is odd.  Every tile and every resumed segment starts on the same parity (its first input in buffer 0).
    auto step = [&](auto XW0, const int t, const bool first) __attribute__((always_inline)) {
        int xw = decltype(XW0)::value;
        CEM_LEAN_PRIO_STEP
#define CEM_RELU_PUBLISH() do { \
            f4 h0 = acc0[0], h1 = acc1[0]; \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) { h0[r] = fmaxf(h0[r], 0.f); h1[r] = fmaxf(h1[r], 0.f); } \
            *reinterpret_cast<f4 *>(pubh + xw) = h0; \
            *reinterpret_cast<f4 *>(pubh + xw + 1024) = h1; \
            hB[0][0] = h0; hB[1][0] = h1; \
            xw ^= XB; } while (0)
#define CEM_NEXT_BIAS(LN) do { \
            nb0 = cem_ld_tab(et_rs, bias_v, (CEM_ET_ROWS + (LN)) * 512); \
            nb1 = cem_ld_tab(et_rs, bias_v + 64, (CEM_ET_ROWS + (LN)) * 512); } while (0)
#define CEM_LEAN_HIDDEN(LN, BASE) { \
            f4 acc0[RC], acc1[RC]; \
            acc0[0] = nb0; acc1[0] = nb1; \
            CEM_NEXT_BIAS(LN); \
            CEM_LEAN_STAGE(CEM_NG, 2, false, BASE)(acc0, acc1, hB, wq, rbh, xw ^ XB); \
            CEM_RELU_PUBLISH(); }
        {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(1);
            CEM_LEAN_STAGE(4, 1, true, 0)(acc0, acc1, hB, wq, rb0, xw ^ XB);
            CEM_LEAN_BOOKS_STEP
            CEM_RELU_PUBLISH();
        }
        CEM_LEAN_HIDDEN_LAYERS
#undef CEM_LEAN_HIDDEN
#undef CEM_RELU_PUBLISH
#undef CEM_NEXT_BIAS

        float pm[2][RC];
        pm[0][0] = __builtin_inff(); pm[1][0] = __builtin_inff();
        const int tn = (t + 1 < H) ? t + 1 : H - 1;
        {
            const int tv = tab_v;
            f4 accm[RC], accv[RC];
            accm[0] = CEM_TAB(tabl, CEM_ET_BMU, tv); accv[0] = CEM_TAB(tabl, CEM_ET_BVAR, tv);
            if (CEM_LEAN_HEADS) CEM_LEAN_STAGE(CEM_NG, 2, false, 28)(accm, accv, hB, wq, rbh, xw ^ XB);
            else __syncthreads();
            // the one draw of the step: model noise, or on the action lanes the next step's action noise
            const f4 e4 = cem_normal4(pc0, pc1 + (uint32_t)t, 0u, pc2, 0u, key, prs);
            const f4 mn4 = CEM_TAB(tabl, CEM_ET_NMIN, tv), rd4 = CEM_TAB(tabl, CEM_ET_RDELTA, tv);
            const f4 om4 = CEM_TAB(tabl, CEM_ET_OBS, tv); CEM_LEAN_ISACT
            const f4 sel0 = CEM_TAB(tabl, CEM_ET_SEL0, tv), sel1 = CEM_TAB(tabl, CEM_ET_SEL1, tv);

            const f4 mu = accm[0];
            const f4 var = cem_softplus4(accv[0]) + 1e-4f;
            f4 sd;
#pragma unroll
            for (int r = 0; r < 4; ++r) sd[r] = __builtin_amdgcn_sqrtf(var[r]);
            const f4 d = mu + sd * e4;                                       // (an action lane's d is masked out: om4 = 0 there)
            const f4 sn = s[0][0] + d * om4;
            s[0][0] = sn;
            cem_scorer_terms(sn, CEM_LEAN_SCORE_D, sel0, sel1, pm[0][0], pm[1][0]);
            CEM_LEAN_NEXT_INPUT
        }
        CEM_LEAN_STORE_TERMS;
    };
    for (int t = t_begin; t < t_end; t += 2) {
        step(LeanConst<XB>{}, t, t == t_begin);
        if (t + 1 >= t_end) break;
        step(LeanConst<0>{}, t + 1, false);
    }
    __syncthreads();
    CEM_LEAN_BOOKS_END
    if (td.row_base < p.Nloc) {                               // (the barrier above published the parked actions)
        const int tlo = resumed ? t_begin + 1 : 0, thi = t_end < H ? t_end : H - 1;      // the steps this tile or segment drew
        const int per = (thi - tlo + 1) * A;
        const float *const stagef = reinterpret_cast<const float *>(stage);
        for (int idx = (int)threadIdx.x; idx < td.cnt * per; idx += 256) {
            const int row = idx / per, rem = idx - row * per, tt = tlo + rem / A, a = rem - (rem / A) * A;
            p.actions_w[((size_t)(td.act_base + row) * H + tt) * A + a] = stagef[((row * (H + 1) + tt) * AZ) * 4 + a];
        }
    }
    if (!SEG || t_end == H) {
        if (CEM_LEAN_BKWAVE && lane < td.cnt) p.ret[td.row_base + lane] = cum;
    } else {
        const __amdgpu_buffer_rsrc_t ho = CEM_LEAN_HANDOVER;
        cem_st_coherent(ho, tid * 16, s[0][0]);
        cem_st_coherent(ho, (256 + tid) * 16, hB[0][0]);
        if (CEM_LEAN_BKWAVE) cem_st_coherent(ho, (2 * 256 + lane) * 16, (f4){d_prev, c_prev, cum, done ? 1.0f : 0.0f});
    }
}
#undef CEM_LEAN_ACTION
#undef CEM_LEAN_KEEP
#undef CEM_LEAN_SEG_RSRC
#undef CEM_LEAN_TILE_TEMPLATE
#undef CEM_LEAN_TILE
#undef CEM_LEAN_HANDOVER_DECL
#undef CEM_LEAN_HANDOVER
#undef CEM_LEAN_BKWAVE
#undef CEM_LEAN_RING
#undef CEM_LEAN_STAGE
#undef CEM_LEAN_BOOKS_DECL
#undef CEM_LEAN_SCORE_D
#undef CEM_LEAN_STORE_TERMS
#undef CEM_LEAN_PRIO_DECL
#undef CEM_LEAN_PRIO_STEP
#undef CEM_LEAN_BOOKS_STEP
#undef CEM_LEAN_BOOKS_END
#undef CEM_LEAN_HIDDEN_LAYERS
#undef CEM_LEAN_HEADS
#undef CEM_LEAN_ISACT
#undef CEM_LEAN_NEXT_INPUT
