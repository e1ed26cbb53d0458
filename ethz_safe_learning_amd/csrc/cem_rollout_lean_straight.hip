// cem_rollout_lean_straight.hip — the straight-line form of the lean one-chunk rollout (cem_rollout_lean.hip is the branchy form): the
// same tile (cem_rollout_lean_tile.h, shared by both), the same instructions on the same data in the same order, for the plans whose
// per-plan facts the host can fix at launch (cem_capi.hip lean_form):
//   - the objective is a template parameter (SAFE: SafeCemMpc's order of done and return, and its cost bytes; else CemMpc's, no bytes);
//   - the scorer has its goal as a lidar kind and at most one constrained cost kind, so the rare kinds and observe_goal_dist are not
//     in the kernel at all, the kind loop is one comparison and the indicator cap is the identity on a count of 0 or 1;
//   - every wave's weight stream is exactly one step long, so the group a ring slot loads next is a compile-time constant: no
//     position register, no compare / select / shift per group, two groups per scalar offset with immediates 0 .. 3072;
//   - the scorer's scalars are read once in front of the loop, the priority level is a counter, and the first step — the only one
//     whose bookkeeping differs — is told apart by one scalar branch.
// Everything else launches the branchy form, which is also this form's bit-exact reference (tests/test_gpu_lean_straight.py).
// Here are the ring and stage with compile-time positions, what this form puts into the tile's hooks, the four kernels and the launcher.
#define CEM_DEVICE_PRIMITIVES_ONLY
#include "cem_rollout_lean.h"

namespace {

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
    group(LeanConst<0>{}); group(LeanConst<1>{}); group(LeanConst<2>{}); group(LeanConst<3>{});
    if constexpr (KF == 8) { group(LeanConst<4>{}); group(LeanConst<5>{}); group(LeanConst<6>{}); group(LeanConst<7>{}); }
}

// The straight-line form's hooks (cem_rollout_lean_tile.h).  The hand-over buffer is built where it is used (in front of the loop and
// behind it), not carried across it.
#define CEM_LEAN_TILE_TEMPLATE template <bool SEG, bool SAFE>
#define CEM_LEAN_TILE cem_straight_tile
#define CEM_LEAN_BKWAVE bkwave
#define CEM_LEAN_HANDOVER_DECL const bool bkwave = w == 0; auto seg_buffer = [&]() __attribute__((always_inline)) { return CEM_LEAN_SEG_RSRC(); };
#define CEM_LEAN_HANDOVER seg_buffer()
#define CEM_LEAN_RING \
    const bool heads = w < p.KB_obs; \
    StraightRing wq; \
    wq.init(p.wpack + (size_t)member_u * p.member_stride_f4 + p.wave_off_f4[w], lane, heads ? SL_GROUPS_HEADS : SL_GROUPS_BODY);
#define CEM_LEAN_STAGE(KF, NOWN, L0IN, BASE) cem_straight_stage<KF, NOWN, L0IN, BASE>
// The scorer's scalars, once.  No second cost kind: kind 1's partial minima are +inf (its selector row is), which no size reaches.
// CEM_BOOKKEEP on the bookkeeping wave for at most two kinds: the terms of the step just published, then step T's reward, cost byte
// and done in the objective's order; the tile's first step only takes d_prev / c_prev from s_0.
#define CEM_LEAN_BOOKS_DECL \
    const float scD = p.sc.D, goal_thresh = p.sc.goal_thresh, reward_distance = p.sc.reward_distance, reward_goal = p.sc.reward_goal; \
    const float clipv = p.sc.reward_clip > 0.f ? p.sc.reward_clip : __builtin_inff(); \
    const float csz0 = p.sc.n_cost > 0 ? p.sc.cost_size[0] : -__builtin_inff(); \
    auto terms = [&](float &dn, float &cn) __attribute__((always_inline)) { \
        dn = CEM_PART_MIN4(part, lane, 0); \
        const float dk = CEM_PART_MIN4(part, lane, 1); \
        cn = (dk <= csz0) ? 1.0f : 0.0f;                      /* (a count of 0 or 1: the indicator cap changes nothing) */ \
    }; \
    auto settle = [&](const float dn, const float cn, const int T) __attribute__((always_inline)) { \
        const bool ga = d_prev <= goal_thresh; \
        float r = (d_prev - dn) * reward_distance + (ga ? 1.0f : 0.0f) * reward_goal; \
        r = fminf(fmaxf(r, -clipv), clipv); \
        if (SAFE) { \
            done = done || ga; \
            const float nd = done ? 0.0f : 1.0f; \
            const float cst = c_prev * nd; \
            if (lane < td.cnt) { \
                const __amdgpu_buffer_rsrc_t cost_rs = __builtin_amdgcn_make_buffer_rsrc(p.costs, 0, (uint32_t)(H * p.Bloc), 0x00020000); \
                __builtin_amdgcn_raw_buffer_store_b8((uint8_t)cst, cost_rs, td.row_base + lane, __builtin_amdgcn_readfirstlane(T * p.Bloc), 0); \
            } \
            cum = cum + r * nd; \
        } else { \
            const float nd = done ? 0.0f : 1.0f; \
            cum = cum + r * nd; \
            done = done || ga; \
        } \
        d_prev = dn; c_prev = cn; \
    };
#define CEM_LEAN_SCORE_D scD
#define CEM_LEAN_STORE_TERMS CEM_PAIR_MIN_STORE(part, w, q, j, 0, pm[0][0], pm[1][0], true, 0)
// the priority rotation's level of step t_begin, a counter from here on: 0 -> 1 -> 2 -> 0; a floating segment stays on level 3,
// CEM_FLOAT_PRIO, which its kernel set (setting it again every step changes nothing and saves the step a test)
#define CEM_LEAN_PRIO_DECL \
    static_assert(CEM_FLOAT_PRIO == 3, "level 3 of the step's priority switch is the floating segments' priority"); \
    int lvl = (SEG && tile_idx >= p.n_pinned) ? 3 : (t_begin + (tile_idx >> 8) % 3) % 3;
#define CEM_LEAN_PRIO_STEP \
    if (lvl < 2) { if (lvl == 0) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(1); } \
    else { if (lvl == 2) __builtin_amdgcn_s_setprio(2); else __builtin_amdgcn_s_setprio(3); } \
    lvl = lvl == 2 ? 0 : (lvl == 3 ? 3 : lvl + 1); \
    asm volatile("" : "+s"(lvl));                           /* (one switch per step: the two half-rounds' switches are not threaded into each other) */
#define CEM_LEAN_BOOKS_STEP \
    if (bkwave) { \
        if (first) { \
            if (!resumed) terms(d_prev, c_prev); \
        } else { \
            float dn, cn; \
            terms(dn, cn); \
            settle(dn, cn, t - 1); \
        } \
    }
#define CEM_LEAN_BOOKS_END \
    if (bkwave) { \
        float dn, cn; \
        terms(dn, cn); \
        settle(dn, cn, t_end - 1); \
    }
#define CEM_LEAN_HIDDEN_LAYERS CEM_LEAN_HIDDEN(2, 4) CEM_LEAN_HIDDEN(3, 12) CEM_LEAN_HIDDEN(0, 20)
#define CEM_LEAN_HEADS heads
#define CEM_LEAN_ISACT
// a wave without an action quad forms the next layer-0 input from sn directly: no copy of it travels round the other branch
#define CEM_LEAN_NEXT_INPUT \
    if (wact) { \
        const f4 isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv); \
        f4 act4; CEM_LEAN_ACTION(act4, e4, tn); \
        CEM_LEAN_KEEP(act4, t + 1); \
        const f4 x = cem_sub4(__builtin_elementwise_fma(isact4, act4, sn), mn4) * rd4; \
        *reinterpret_cast<f4 *>(pub0 + xw) = x; \
        hB[0][0] = x; \
    } else { \
        const f4 x = cem_sub4(sn, mn4) * rd4; \
        *reinterpret_cast<f4 *>(pub0 + xw) = x; \
        hB[0][0] = x; \
    }
#include "cem_rollout_lean_tile.h"

}  // namespace

template <bool SAFE>
__global__ __launch_bounds__(256) void cem_rollout_lean_straight_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_straight_tile<false, SAFE>(p, smem, (int)blockIdx.x, 0, p.H);
}

// cem_rollout_lean_seg_kernel's tickets, FIFO and hand-over (CEM_SEG_SCHEDULE, cem_device.h) around the straight-line tile
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
    CEM_SEG_SCHEDULE(p, item_s, tile, seg, t0, t1, (cem_straight_tile<true, SAFE>(p, smem, tile, t0, t1)))
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
