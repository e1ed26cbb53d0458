// cem_rollout_lean_straight.hip — the straight-line form of the lean one-chunk rollout (cem_rollout_lean.hip, the branchy form, whose
// comments apply and are not repeated): the same tile, the same instructions on the same data in the same order, for the plans whose
// per-plan facts the host can fix at launch (cem_capi.hip lean_form):
//   - the objective is a template parameter (SAFE: SafeCemMpc's order of done and return, and its cost bytes; else CemMpc's, no bytes);
//   - the scorer has its goal as a lidar kind and at most one constrained cost kind, so the rare kinds and observe_goal_dist are not
//     in the kernel at all, the kind loop is one comparison and the indicator cap is the identity on a count of 0 or 1;
//   - every wave's weight stream is exactly one step long, so the group a ring slot loads next is a compile-time constant: no
//     position register, no compare / select / shift per group, two groups per scalar offset with immediates 0 .. 3072;
//   - the scorer's scalars are read once in front of the loop, the priority level is a counter, and the first step — the only one
//     whose bookkeeping differs — is told apart by one scalar branch.
// Everything else launches the branchy form, which is also this form's bit-exact reference (tests/test_gpu_lean_straight.py).
// A translation unit of its own: cem_rollout_lean.hip stays the two branchy kernels to the byte.
#define CEM_DEVICE_PRIMITIVES_ONLY
#include "cem_rollout_lean.h"

namespace {

template <int V> struct StraightConst { static constexpr int value = V; };

// groups a wave's stream holds per step without / with the heads stage (layer 0: 4, three hidden layers: 8 each, the heads: 8)
constexpr int SL_GROUPS_BODY = 4 + 3 * CEM_NG, SL_GROUPS_HEADS = SL_GROUPS_BODY + CEM_NG;

// WRing with the position known at compile time.  Group G of the step (counted from the step's first) is group G of the stream, or —
// the three loads that run ahead into the next step — group G - n; n is 28 or 36, both even, so the half of the 4 KB pair is G's own.
struct StraightRing {
    __amdgpu_buffer_rsrc_t rsrc;
    int voff, n;
    AGroup slot[4];
    template <int G> __device__ __forceinline__ AGroup ld() const
    {
        const int g = G < SL_GROUPS_BODY ? G : (G >= n ? G - n : G);
        const int soff = (g >> 1) * 4096;
        constexpr int half = (G & 1) * 2048;
        AGroup r;
        r.a = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + half, soff, 0));
        r.b = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + half + 1024, soff, 0));
        return r;
    }
    __device__ __forceinline__ void init(const f4 *b, int lane_, int n_)
    {
        rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<f4 *>(b), 0, n_ * 2048, 0x00020000);
        voff = lane_ * 16; n = n_;
        slot[0] = ld<0>(); slot[1] = ld<1>(); slot[2] = ld<2>(); slot[3] = slot[2];
    }
};

// cem_lean_stage with the ring position BASE + P (BASE: the groups of the step in front of this stage)
template <int KF, int NOWN, bool L0IN, int BASE>
__device__ __forceinline__ void cem_straight_stage(f4 (&acc0)[1], f4 (&acc1)[1], f4 (&hB)[CEM_NG][1], StraightRing &wq, const char *const *rb, const int xoff)
{
    static_assert(KF % 4 == 0 && BASE % 4 == 0, "stage lengths must keep the ring phase");
    auto group = [&](auto PC) __attribute__((always_inline)) {
        constexpr int P = decltype(PC)::value;
        wq.slot[(P + 3) & 3] = wq.template ld<BASE + P + 3>();
        __builtin_amdgcn_sched_barrier(0);
        if (P == 1) {
            __syncthreads();
#pragma unroll
            for (int Q = NOWN; Q < KF; ++Q) hB[Q][0] = *reinterpret_cast<const f4 *>(rb[Q - NOWN] + xoff + (Q - NOWN) * 1024);
        }
        const AGroup g = wq.slot[P & 3];
        constexpr int Pb = (!L0IN && P < 2) ? (P ^ 1) : P;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            acc0[0] = CEM_MFMA(g.a[r], hB[P][0][r], acc0[0]);
            acc1[0] = CEM_MFMA(g.b[r], hB[Pb][0][r], acc1[0]);
        }
    };
    group(StraightConst<0>{}); group(StraightConst<1>{}); group(StraightConst<2>{}); group(StraightConst<3>{});
    if constexpr (KF == 8) { group(StraightConst<4>{}); group(StraightConst<5>{}); group(StraightConst<6>{}); group(StraightConst<7>{}); }
}

template <bool SEG, bool SAFE>
__device__ __forceinline__ void cem_straight_tile(const RolloutParams &p, char *smem, const int tile_idx, const int t_begin, const int t_end)
{
    constexpr int RC = 1;
    const int tid = (int)((threadIdx.x + 64u * (unsigned)((tile_idx + (tile_idx >> 8)) & 3)) & 255u);
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lane = tid & 63;
    const int j = lane & 15, q = lane >> 4;
    const TileDesc td = p.tiles[tile_idx];
    const bool resumed = SEG && t_begin > 0;
    const bool bkwave = w == 0;
    // the hand-over buffer, built where it is used (in front of the loop and behind it), not carried across it
    auto seg_buffer = [&]() __attribute__((always_inline)) {
        return __builtin_amdgcn_make_buffer_rsrc(
            SEG ? const_cast<f4 *>(p.seg_state + (size_t)(tile_idx - p.n_pinned) * (2 * 256 + 64)) : const_cast<f4 *>(p.wpack), 0, (2 * 256 + 64) * 16, 0x00020000);
    };
    const int O = p.O, A = p.A, H = p.H, AZ = (A + 3) >> 2;
    constexpr int XB = CEM_NG * 1024;
    float *part = reinterpret_cast<float *>(smem + 2 * XB);
    const CtrlBlock *const ctrl = p.ctrl;
    const PhiloxKey key = cem_key(ctrl);
    const float rscale = p.sampling ? CEM_BM_RSCALE : 0.0f;

    const int member_u = __builtin_amdgcn_readfirstlane(td.member);
    const bool heads = w < p.KB_obs;
    StraightRing wq;
    wq.init(p.wpack + (size_t)member_u * p.member_stride_f4 + p.wave_off_f4[w], lane, heads ? SL_GROUPS_HEADS : SL_GROUPS_BODY);

    const __amdgpu_buffer_rsrc_t et_rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(p.etab + (size_t)member_u * (CEM_ET_ROWS + p.L) * CEM_U), 0, (CEM_ET_ROWS + p.L) * CEM_U * 4, 0x00020000);
    const int tab_v = 64 * w + 16 * q;
    const int bias_v = 128 * w + 16 * q;
    const char *tabl = smem + 2 * XB + CEM_PART_FLOATS * 4;
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

    f4 s;
    const int slot0 = j < td.cnt ? j : td.cnt - 1;
    {
        const int f0 = 16 * w + 4 * q;
        if (resumed) s = cem_ld_coherent(seg_buffer(), tid * 16);
        else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = f0 + r;
                float v = 0.f;
                if (f < O) v = td.s0_base < 0 ? ctrl->state[f] : p.s0[(size_t)(td.s0_base + slot0) * O + f];
                s[r] = v;
            }
        }
    }

    const int zq = 4 * w + q - (O >> 2);
    const bool actlane = zq >= 0 && zq < AZ;
    const bool wact = 4 * w + 3 >= (O >> 2) && 4 * w < (O >> 2) + AZ;
    const int zc = actlane ? zq : 0;
    const uint32_t pc0 = (uint32_t)((actlane ? td.act_base : td.noise_row_base) + slot0);
    const uint32_t pc2 = actlane ? ((uint32_t)zc | (CEM_STREAM_ACT << 16)) : ((uint32_t)(4 * w + q) | (CEM_STREAM_MODEL << 16));
    const uint32_t pc1 = ((uint32_t)p.it << 16) + (actlane ? 1u : 0u);
    const float prs = actlane ? CEM_BM_RSCALE : rscale;
    const char *const actl_v = actl + zc * 32;
#define CEM_LEAN_ACTION(DST, E_, T_) do { \
        const char *m_ = actl_v + (T_) * AZ * 32, *b_ = actl_v + H * AZ * 32; \
        const f4 sg_ = *reinterpret_cast<const f4 *>(m_), mu_ = *reinterpret_cast<const f4 *>(m_ + 16); \
        const f4 lb_ = *reinterpret_cast<const f4 *>(b_), ub_ = *reinterpret_cast<const f4 *>(b_ + 16); \
        f4 v_ = (E_) * sg_; v_ = v_ + mu_; \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) DST[r] = fminf(fmaxf(v_[r], lb_[r]), ub_[r]); } while (0)
    const bool act_keep = actlane && j < td.cnt && td.row_base < p.Nloc;
    char *const stage = const_cast<char *>(actl) + (H + 1) * AZ * 32;
    char *const stage_v = stage + ((act_keep ? j : 16) * (H + 1) * AZ + zc) * 16;
#define CEM_LEAN_KEEP(V_, T_) do { *reinterpret_cast<f4 *>(stage_v + (T_) * AZ * 16) = (V_); } while (0)

    // the scorer's scalars, once.  No second cost kind: kind 1's partial minima are +inf (its selector row is), which no size reaches
    const float scD = p.sc.D, goal_thresh = p.sc.goal_thresh, reward_distance = p.sc.reward_distance, reward_goal = p.sc.reward_goal;
    const float clipv = p.sc.reward_clip > 0.f ? p.sc.reward_clip : __builtin_inff();
    const float csz0 = p.sc.n_cost > 0 ? p.sc.cost_size[0] : -__builtin_inff();
    float d_prev = 0.f, c_prev = 0.f, cum = 0.f;
    bool done = false;

    // CEM_BOOKKEEP on the bookkeeping wave for at most two kinds: the terms of the step just published, then (FULL) step T's reward,
    // cost byte and done in the objective's order; the tile's first step only takes d_prev / c_prev from s_0
    auto terms = [&](float &dn, float &cn) __attribute__((always_inline)) {
        dn = CEM_PART_MIN4(part, lane, 0);
        const float dk = CEM_PART_MIN4(part, lane, 1);
        cn = (dk <= csz0) ? 1.0f : 0.0f;                      // (a count of 0 or 1: the indicator cap changes nothing)
    };
    auto settle = [&](const float dn, const float cn, const int T) __attribute__((always_inline)) {
        const bool ga = d_prev <= goal_thresh;
        float r = (d_prev - dn) * reward_distance + (ga ? 1.0f : 0.0f) * reward_goal;
        r = fminf(fmaxf(r, -clipv), clipv);
        if (SAFE) {
            done = done || ga;
            const float nd = done ? 0.0f : 1.0f;
            const float cst = c_prev * nd;
            if (lane < td.cnt) {
                const __amdgpu_buffer_rsrc_t cost_rs = __builtin_amdgcn_make_buffer_rsrc(p.costs, 0, (uint32_t)(H * p.Bloc), 0x00020000);
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)cst, cost_rs, td.row_base + lane, __builtin_amdgcn_readfirstlane(T * p.Bloc), 0);
            }
            cum = cum + r * nd;
        } else {
            const float nd = done ? 0.0f : 1.0f;
            cum = cum + r * nd;
            done = done || ga;
        }
        d_prev = dn; c_prev = cn;
    };

    f4 hB[CEM_NG][RC];
    if (resumed) {
        const __amdgpu_buffer_rsrc_t seg_rs = seg_buffer();
        const f4 x = cem_ld_coherent(seg_rs, (256 + tid) * 16);
        hB[0][0] = x;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        if (bkwave) {
            const f4 b = cem_ld_coherent(seg_rs, (2 * 256 + lane) * 16);
            d_prev = b[0]; c_prev = b[1]; cum = b[2]; done = b[3] != 0.f;
        }
    } else {
        float pm0 = __builtin_inff(), pm1 = __builtin_inff();
        const int tv = tab_v;
        const f4 mn4 = CEM_TAB(tabl, CEM_ET_NMIN, tv), rd4 = CEM_TAB(tabl, CEM_ET_RDELTA, tv);
        const f4 isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv);
        const f4 sel0 = CEM_TAB(tabl, CEM_ET_SEL0, tv), sel1 = CEM_TAB(tabl, CEM_ET_SEL1, tv);
        const f4 e0 = cem_normal4(pc0, 0u, (uint32_t)p.it, (uint32_t)zc, CEM_STREAM_ACT, key);
        const f4 sn = s;
        f4 xin = sn;
        if (wact) {
            f4 act4; CEM_LEAN_ACTION(act4, e0, 0);
            CEM_LEAN_KEEP(act4, 0);
            xin = __builtin_elementwise_fma(isact4, act4, sn);
        }
        cem_scorer_terms(sn, scD, sel0, sel1, pm0, pm1);
        const f4 x = cem_sub4(xin, mn4) * rd4;
        *reinterpret_cast<f4 *>(smem + (w * 64 + lane) * 16) = x;
        hB[0][0] = x;
        CEM_PAIR_MIN_STORE(part, w, q, j, 0, pm0, pm1, true, 0);
    }
    f4 nb0 = cem_ld_tab(et_rs, bias_v, CEM_ET_ROWS * 512);
    f4 nb1 = cem_ld_tab(et_rs, bias_v + 64, CEM_ET_ROWS * 512);

    const char *rbh[6], *rb0[3];
#pragma unroll
    for (int k = 0; k < 6; ++k) rbh[k] = smem + lane * 16 + (k < 2 * w ? 0 : 2048);
#pragma unroll
    for (int k = 0; k < 3; ++k) rb0[k] = smem + lane * 16 + (k < w ? 0 : 1024);
    char *const pubh = smem + (2 * w * 64 + lane) * 16, *const pub0 = smem + (w * 64 + lane) * 16;
    // the priority rotation's level of step t_begin, a counter from here on: 0 -> 1 -> 2 -> 0; a floating segment stays on level 3,
    // CEM_FLOAT_PRIO, which its kernel set (setting it again every step changes nothing and saves the step a test)
    static_assert(CEM_FLOAT_PRIO == 3, "level 3 of the step's priority switch is the floating segments' priority");
    int lvl = (SEG && tile_idx >= p.n_pinned) ? 3 : (t_begin + (tile_idx >> 8) % 3) % 3;
    auto step = [&](auto XW0, const int t, const bool first) __attribute__((always_inline)) {
        int xw = decltype(XW0)::value;
        if (lvl < 2) { if (lvl == 0) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(1); }
        else { if (lvl == 2) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3); }
        lvl = lvl == 2 ? 0 : (lvl == 3 ? 3 : lvl + 1);
        asm volatile("" : "+s"(lvl));                           // (one switch per step: the two half-rounds' switches are not threaded into each other)
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
            cem_straight_stage<4, 1, true, 0>(acc0, acc1, hB, wq, rb0, xw ^ XB);
            if (bkwave) {
                if (first) {
                    if (!resumed) terms(d_prev, c_prev);
                } else {
                    float dn, cn;
                    terms(dn, cn);
                    settle(dn, cn, t - 1);
                }
            }
            CEM_RELU_PUBLISH();
        }
        {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(2);
            cem_straight_stage<CEM_NG, 2, false, 4>(acc0, acc1, hB, wq, rbh, xw ^ XB);
            CEM_RELU_PUBLISH();
        }
        {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(3);
            cem_straight_stage<CEM_NG, 2, false, 12>(acc0, acc1, hB, wq, rbh, xw ^ XB);
            CEM_RELU_PUBLISH();
        }
        {
            f4 acc0[RC], acc1[RC];
            acc0[0] = nb0; acc1[0] = nb1;
            CEM_NEXT_BIAS(0);
            cem_straight_stage<CEM_NG, 2, false, 20>(acc0, acc1, hB, wq, rbh, xw ^ XB);
            CEM_RELU_PUBLISH();
        }
#undef CEM_RELU_PUBLISH
#undef CEM_NEXT_BIAS

        float pm0 = __builtin_inff(), pm1 = __builtin_inff();
        const int tn = (t + 1 < H) ? t + 1 : H - 1;
        {
            const int tv = tab_v;
            f4 accm[RC], accv[RC];
            accm[0] = CEM_TAB(tabl, CEM_ET_BMU, tv); accv[0] = CEM_TAB(tabl, CEM_ET_BVAR, tv);
            if (heads) cem_straight_stage<CEM_NG, 2, false, 28>(accm, accv, hB, wq, rbh, xw ^ XB);
            else __syncthreads();
            const f4 e4 = cem_normal4(pc0, pc1 + (uint32_t)t, 0u, pc2, 0u, key, prs);
            const f4 mn4 = CEM_TAB(tabl, CEM_ET_NMIN, tv), rd4 = CEM_TAB(tabl, CEM_ET_RDELTA, tv);
            const f4 om4 = CEM_TAB(tabl, CEM_ET_OBS, tv);
            const f4 sel0 = CEM_TAB(tabl, CEM_ET_SEL0, tv), sel1 = CEM_TAB(tabl, CEM_ET_SEL1, tv);

            const f4 mu = accm[0];
            const f4 var = cem_softplus4(accv[0]) + 1e-4f;
            f4 sd;
#pragma unroll
            for (int r = 0; r < 4; ++r) sd[r] = __builtin_amdgcn_sqrtf(var[r]);
            const f4 d = mu + sd * e4;
            const f4 sn = s + d * om4;
            s = sn;
            cem_scorer_terms(sn, scD, sel0, sel1, pm0, pm1);
            // a wave without an action quad forms the next layer-0 input from sn directly: no copy of it travels round the other branch
            if (wact) {
                const f4 isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv);
                f4 act4; CEM_LEAN_ACTION(act4, e4, tn);
                CEM_LEAN_KEEP(act4, t + 1);
                const f4 x = cem_sub4(__builtin_elementwise_fma(isact4, act4, sn), mn4) * rd4;
                *reinterpret_cast<f4 *>(pub0 + xw) = x;
                hB[0][0] = x;
            } else {
                const f4 x = cem_sub4(sn, mn4) * rd4;
                *reinterpret_cast<f4 *>(pub0 + xw) = x;
                hB[0][0] = x;
            }
        }
        CEM_PAIR_MIN_STORE(part, w, q, j, 0, pm0, pm1, true, 0);
    };
    for (int t = t_begin; t < t_end; t += 2) {
        step(StraightConst<XB>{}, t, t == t_begin);
        if (t + 1 >= t_end) break;
        step(StraightConst<0>{}, t + 1, false);
    }
#undef CEM_LEAN_ACTION
#undef CEM_LEAN_KEEP
    __syncthreads();
    if (bkwave) {
        float dn, cn;
        terms(dn, cn);
        settle(dn, cn, t_end - 1);
    }
    if (td.row_base < p.Nloc) {
        const int tlo = resumed ? t_begin + 1 : 0, thi = t_end < H ? t_end : H - 1;
        const int per = (thi - tlo + 1) * A;
        const float *const stagef = reinterpret_cast<const float *>(stage);
        for (int idx = (int)threadIdx.x; idx < td.cnt * per; idx += 256) {
            const int row = idx / per, rem = idx - row * per, tt = tlo + rem / A, a = rem - (rem / A) * A;
            p.actions_w[((size_t)(td.act_base + row) * H + tt) * A + a] = stagef[((row * (H + 1) + tt) * AZ) * 4 + a];
        }
    }
    if (!SEG || t_end == H) {
        if (bkwave && lane < td.cnt) p.ret[td.row_base + lane] = cum;
    } else {
        const __amdgpu_buffer_rsrc_t seg_rs = seg_buffer();
        cem_st_coherent(seg_rs, tid * 16, s);
        cem_st_coherent(seg_rs, (256 + tid) * 16, hB[0][0]);
        if (bkwave) cem_st_coherent(seg_rs, (2 * 256 + lane) * 16, (f4){d_prev, c_prev, cum, done ? 1.0f : 0.0f});
    }
}

}  // namespace

template <bool SAFE>
__global__ __launch_bounds__(256) void cem_rollout_lean_straight_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_straight_tile<false, SAFE>(p, smem, (int)blockIdx.x, 0, p.H);
}

// cem_rollout_lean_seg_kernel's tickets, FIFO and hand-over (the same protocol on the same words) around the straight-line tile
template <bool SAFE>
__global__ __launch_bounds__(256) void cem_rollout_lean_straight_seg_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t item_s;
    if (p.check_done && p.ctrl->done) return;
    if ((int)blockIdx.x < p.n_pinned) {
        cem_straight_tile<true, SAFE>(p, smem, (int)blockIdx.x, 0, p.H);
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
    cem_straight_tile<true, SAFE>(p, smem, tile, t0, t1);
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
        __builtin_amdgcn_s_waitcnt(0x0F70);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t pos = atomicAdd(p.seg_queue + 1, 1u);
            __hip_atomic_store(p.seg_flags + pos, (((uint32_t)tile << 8) | (uint32_t)(seg + 1)) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

hipError_t launch_rollout_lean_straight(const RolloutParams &p, int grid, hipStream_t st, bool seg)
{
    const size_t lds = CEM_LEAN_LDS_BYTES(p.H, (p.A + 3) / 4);
    const bool safe = p.variant == 1;
    if (seg) {
        if (safe) hipLaunchKernelGGL(cem_rollout_lean_straight_seg_kernel<true>, dim3(grid), dim3(256), lds, st, p);
        else hipLaunchKernelGGL(cem_rollout_lean_straight_seg_kernel<false>, dim3(grid), dim3(256), lds, st, p);
    } else {
        if (safe) hipLaunchKernelGGL(cem_rollout_lean_straight_kernel<true>, dim3(grid), dim3(256), lds, st, p);
        else hipLaunchKernelGGL(cem_rollout_lean_straight_kernel<false>, dim3(grid), dim3(256), lds, st, p);
    }
    return hipGetLastError();
}
