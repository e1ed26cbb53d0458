// cem_rollout_lean.hip — the planner's one-chunk fp32 rollout (cem_rollout_tile at RC = 1, NFW = 1, MODE 0: obs + act <= 64, Philox noise)
// without a materialised action sample.
//
// cem_rollout_tile draws one cem_normal4 per lane and step for the model noise.  The lanes whose feature quad holds the ACTION features
// (obs 60: block 3, q = 3) multiply that draw by the observation mask, 0.  Philox is counter based, so here those lanes draw the action
// noise of (candidate, t + 1) with the same call instead — the counter words are per-lane registers fixed before the step loop — and form
// a = clip(eps * sigma + mu, lb, ub) in the epilogue, where the generic kernel loads the quad cem_tile_sample_actions stored.  The
// sampler prologue, its two stores per draw, their vmcnt(0) drain and the 16-byte action load of every step are gone; the tiles of
// particle 0 store their rows' actions into the natural [N][H][A] array (what the select and cem_planner_actions read), the padded quad
// array is neither written nor read.  Same counters, same roundings: bit-identical to the generic kernels (tests/test_gpu_lean_rollout.py).
// The path also requires depth 4, which lets the step loop run two steps per round with every LDS offset of the activation exchange a
// compile-time constant (cem_lean_stage, and the loop at the end of cem_lean_tile).
// Eligibility is decided on the host (cem_capi.hip lean_eligible); O % 4 == 0 makes every feature quad all-observation or all-action.
#define CEM_DEVICE_PRIMITIVES_ONLY
#include "cem_rollout_lean.h"

namespace {

template <int V> struct LeanConst { static constexpr int value = V; };

// cem_mfma_stage at RC = 1 with all the other waves' blocks read right behind the barrier (its LA = 6 form), and with LDS addresses
// whose run-time part is loop invariant: block Q of the stage is read at rb[Q - NOWN] + xoff + (Q - NOWN) * 1024, where rb[] holds
// the lane and the wave's role (which blocks it skips as its own) and xoff — the exchange buffer — is a compile-time constant once
// the step loop is unrolled by two (below).  Same groups, same MFMA order as cem_mfma_stage: bit-identical sums.
template <int KF, int NOWN, bool L0IN>
__device__ __forceinline__ void cem_lean_stage(f4 (&acc0)[1], f4 (&acc1)[1], f4 (&hB)[CEM_NG][1], WRing &wq, const char *const *rb, const int xoff)
{
    static_assert(KF % 4 == 0, "stage lengths must keep the ring phase");
#pragma unroll
    for (int P = 0; P < KF; ++P) {
        wq.slot[(P + 3) & 3] = wq.ld(wq.pos);
        wq.pos = (wq.pos + 1 == wq.n) ? 0 : wq.pos + 1;
        __builtin_amdgcn_sched_barrier(0);
        if (P == 1) {
            __syncthreads();
#pragma unroll
            for (int Q = NOWN; Q < KF; ++Q) hB[Q][0] = *reinterpret_cast<const f4 *>(rb[Q - NOWN] + xoff + (Q - NOWN) * 1024);
        }
        const AGroup g = wq.slot[P & 3];
        const int Pb = (!L0IN && P < 2) ? (P ^ 1) : P;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc0[0] = CEM_MFMA(g.a[r], hB[P][0][r], acc0[0]);
            acc1[0] = CEM_MFMA(g.b[r], hB[Pb][0][r], acc1[0]);
        }
    }
}

// One tile for steps [t_begin, t_end): cem_rollout_tile<1, 1, 0, SEG> — the weight ring, stage order, barriers per step, priority
// rotation, bookkeeping and hand-over are that function's; the comments there apply and are not repeated.
template <bool SEG>
__device__ __forceinline__ void cem_lean_tile(const RolloutParams &p, char *smem, const int tile_idx, const int t_begin, const int t_end)
{
    constexpr int RC = 1, NFW = 1;
    const int tid = (int)((threadIdx.x + 64u * (unsigned)((tile_idx + (tile_idx >> 8)) & 3)) & 255u);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int j = lane & 15, q = lane >> 4;
    const TileDesc td = p.tiles[tile_idx];
    const bool resumed = SEG && t_begin > 0;
    const int wbk = 0;
    const __amdgpu_buffer_rsrc_t seg_rs = __builtin_amdgcn_make_buffer_rsrc(
        SEG ? const_cast<f4 *>(p.seg_state + (size_t)(tile_idx - p.n_pinned) * (2 * 256 + 64)) : const_cast<f4 *>(p.wpack), 0, (2 * 256 + 64) * 16, 0x00020000);
    const int O = p.O, A = p.A, H = p.H, AZ = (A + 3) >> 2;
    constexpr int XB = CEM_NG * 1024;
    float *part = reinterpret_cast<float *>(smem + 2 * XB);
    const CtrlBlock *const ctrl = p.ctrl;
    const PhiloxKey key = cem_key(ctrl);
    const float rscale = p.sampling ? CEM_BM_RSCALE : 0.0f;

    const int member_u = __builtin_amdgcn_readfirstlane(td.member);
    WRing wq;
    wq.init(p.wpack + (size_t)member_u * p.member_stride_f4 + p.wave_off_f4[w], lane, (int)p.wave_groups[w]);

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
        if (resumed) s[0][0] = cem_ld_coherent(seg_rs, tid * 16);
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
    const int nk = 1 + p.sc.n_cost;
    const float csz[4] = {p.sc.cost_size[0], p.sc.cost_size[1], p.sc.cost_size[2], p.sc.cost_size[3]};
    const float ind_cap = p.sc.indicator ? 1.0f : __builtin_inff(), clipv = p.sc.reward_clip > 0.f ? p.sc.reward_clip : __builtin_inff();
    const __amdgpu_buffer_rsrc_t cost_rs = __builtin_amdgcn_make_buffer_rsrc(p.costs, 0, p.costs ? (uint32_t)(H * p.Bloc) : 0u, 0x00020000);

    f4 hB[CEM_NG][RC];
    if (resumed) {
        // (the hand-over carries the next layer-0 input, the action of step t_begin inside it: nothing is drawn again)
        const f4 x = cem_ld_coherent(seg_rs, (256 + tid) * 16);
        hB[0][0] = x;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        if (w == wbk) {
            const f4 b = cem_ld_coherent(seg_rs, (2 * 256 + lane) * 16);
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
        cem_scorer_terms(sn, p.sc.D, sel0, sel1, pm[0][0], pm[1][0]);
        const f4 x = cem_sub4(xin, mn4) * rd4;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        hB[0][0] = x;
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_LDS, tabl);
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
    const bool prio_rot = !(SEG && tile_idx >= p.n_pinned);
    const int prio_r0 = (tile_idx >> 8) % 3;
    // The exchange buffer toggles five times a step (depth 4: layer 0, three hidden layers, the heads; lean_eligible), so its parity
    // alternates with the step: the loop runs two steps per round, each with the buffer offsets as compile-time constants, and leaves
    // between them when the count is odd.  Every tile and every resumed segment starts on the same parity (its first input in buffer 0).
    auto step = [&](auto XW0, const int t, const bool first) __attribute__((always_inline)) {
        int xw = decltype(XW0)::value;
        if (prio_rot) {
            const int lvl = (t + prio_r0) % 3;
            if (lvl == 0) __builtin_amdgcn_s_setprio(0); else if (lvl == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2);
        }
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
        {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(1);
            cem_lean_stage<4, 1, true>(acc0, acc1, hB, wq, rb0, xw ^ XB);
            if (!(resumed && first)) CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, t - 1);
            CEM_RELU_PUBLISH();
        }
#pragma unroll
        for (int l = 1; l < 4; ++l) {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(l + 1 < 4 ? l + 1 : 0);
            cem_lean_stage<CEM_NG, 2, false>(acc0, acc1, hB, wq, rbh, xw ^ XB);
            CEM_RELU_PUBLISH();
        }
#undef CEM_RELU_PUBLISH
#undef CEM_NEXT_BIAS

        float pm[2][RC];
        pm[0][0] = __builtin_inff(); pm[1][0] = __builtin_inff();
        const int tn = (t + 1 < H) ? t + 1 : H - 1;
        {
            const int Fo = w;
            const int tv = tab_v;
            f4 accm[RC], accv[RC];
            accm[0] = CEM_TAB(tabl, CEM_ET_BMU, tv); accv[0] = CEM_TAB(tabl, CEM_ET_BVAR, tv);
            if (Fo < p.KB_obs) cem_lean_stage<CEM_NG, 2, false>(accm, accv, hB, wq, rbh, xw ^ XB);
            else __syncthreads();
            // the one draw of the step: model noise, or on the action lanes the next step's action noise
            const f4 e4 = cem_normal4(pc0, pc1 + (uint32_t)t, 0u, pc2, 0u, key, prs);
            const f4 mn4 = CEM_TAB(tabl, CEM_ET_NMIN, tv), rd4 = CEM_TAB(tabl, CEM_ET_RDELTA, tv);
            const f4 om4 = CEM_TAB(tabl, CEM_ET_OBS, tv), isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv);
            const f4 sel0 = CEM_TAB(tabl, CEM_ET_SEL0, tv), sel1 = CEM_TAB(tabl, CEM_ET_SEL1, tv);

            const f4 mu = accm[0];
            const f4 var = cem_softplus4(accv[0]) + 1e-4f;
            f4 sd;
#pragma unroll
            for (int r = 0; r < 4; ++r) sd[r] = __builtin_amdgcn_sqrtf(var[r]);
            const f4 d = mu + sd * e4;                                       // (an action lane's d is masked out: om4 = 0 there)
            const f4 sn = s[0][0] + d * om4;
            s[0][0] = sn;
            cem_scorer_terms(sn, p.sc.D, sel0, sel1, pm[0][0], pm[1][0]);
            f4 xin = sn;
            if (wact) {
                f4 act4; CEM_LEAN_ACTION(act4, e4, tn);
                CEM_LEAN_KEEP(act4, t + 1);
                xin = __builtin_elementwise_fma(isact4, act4, sn);
            }
            const f4 x = cem_sub4(xin, mn4) * rd4;
            *reinterpret_cast<f4 *>(pub0 + xw) = x;
            hB[0][0] = x;
        }
        CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_LDS, tabl);
    };
    for (int t = t_begin; t < t_end; t += 2) {
        step(LeanConst<XB>{}, t, t == t_begin);
        if (t + 1 >= t_end) break;
        step(LeanConst<0>{}, t + 1, false);
    }
#undef CEM_LEAN_ACTION
#undef CEM_LEAN_KEEP
    __syncthreads();
    CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, t_end - 1);
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
        if (w == wbk && lane < td.cnt) p.ret[td.row_base + lane] = cum;
    } else {
        cem_st_coherent(seg_rs, tid * 16, s[0][0]);
        cem_st_coherent(seg_rs, (256 + tid) * 16, hB[0][0]);
        if (w == wbk) cem_st_coherent(seg_rs, (2 * 256 + lane) * 16, (f4){d_prev, c_prev, cum, done ? 1.0f : 0.0f});
    }
}

}  // namespace

// one workgroup per tile, the whole horizon
__global__ __launch_bounds__(256) void cem_rollout_lean_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_lean_tile<false>(p, smem, (int)blockIdx.x, 0, p.H);
}

// Pinned tiles + floating segments: cem_rollout_seg_kernel's tickets, FIFO and hand-over around the lean tile (the comments there apply).
// A segment hands its successor the next layer-0 input, which holds the action of the successor's first step: nothing sampled crosses.
__global__ __launch_bounds__(256) void cem_rollout_lean_seg_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t item_s;
    if (p.check_done && p.ctrl->done) return;
    if ((int)blockIdx.x < p.n_pinned) {
        cem_lean_tile<true>(p, smem, (int)blockIdx.x, 0, p.H);
        return;
    }
    __builtin_amdgcn_s_setprio(CEM_FLOAT_PRIO);
    const uint32_t n_float = (uint32_t)(p.n_tiles - p.n_pinned);
    if (threadIdx.x == 0) {
        const uint32_t ticket = atomicAdd(p.seg_queue, 1u);
        uint32_t item = (((uint32_t)p.n_pinned + ticket) << 8);
        if (ticket >= n_float) {
            const uint32_t *slot = p.seg_flags + (ticket - n_float);
            uint32_t spins = 0, v;
            while ((v = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u && ++spins < CEM_SEG_SPIN_LIMIT)
                __builtin_amdgcn_s_sleep(16);
            item = v ? v - 1u : 0xffffffffu;
            if (!v) atomicOr(const_cast<int32_t *>(&p.ctrl->fault), 1 /* CEM_FAULT_SEGMENT */);
        }
        item_s = item;
    }
    __syncthreads();
    const uint32_t item = item_s;
    if (item == 0xffffffffu) return;
    const int tile = (int)(item >> 8), seg = (int)(item & 255u);
    const int t0 = seg * p.seg_len, t1 = (t0 + p.seg_len < p.H) ? t0 + p.seg_len : p.H;
    cem_lean_tile<true>(p, smem, tile, t0, t1);
    if (t1 == p.H) {
        if (threadIdx.x == 0) item_s = atomicAdd(p.seg_queue + 2, 1u);
        __syncthreads();
        if (item_s == n_float - 1u) {
            const int n_ready = (int)n_float * (p.n_seg - 1);
            for (int i = (int)threadIdx.x; i < n_ready; i += 256) __hip_atomic_store(p.seg_flags + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (threadIdx.x < 3) __hip_atomic_store(p.seg_queue + threadIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (t1 < p.H) {
        // every wave waits for its own sc1 state stores (vmcnt(0)) before the barrier that precedes the flag
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t pos = atomicAdd(p.seg_queue + 1, 1u);
            __hip_atomic_store(p.seg_flags + pos, (((uint32_t)tile << 8) | (uint32_t)(seg + 1)) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

hipError_t launch_rollout_lean(const RolloutParams &p, int grid, hipStream_t st, bool seg)
{
    const size_t lds = CEM_LEAN_LDS_BYTES(p.H, (p.A + 3) / 4);
    if (seg) hipLaunchKernelGGL(cem_rollout_lean_seg_kernel, dim3(grid), dim3(256), lds, st, p);
    else hipLaunchKernelGGL(cem_rollout_lean_kernel, dim3(grid), dim3(256), lds, st, p);
    return hipGetLastError();
}
