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
// This unit is the BRANCHY form of that tile: the bit-exact reference of the straight-line form (cem_rollout_lean_straight.hip) and
// the fallback for goal_mode, two cost kinds and CEM_FORCE_ROLLOUT=lean_branchy.  The tile itself is cem_rollout_lean_tile.h, shared
// with the straight-line form; here are the ring stage, what this form puts into the tile's hooks, the two kernels and the launcher.
#define CEM_DEVICE_PRIMITIVES_ONLY
#include "cem_rollout_lean.h"

namespace {

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

// The branchy form's hooks (cem_rollout_lean_tile.h): the hand-over descriptor is built once; WRing and cem_lean_stage; the generic
// bookkeeper and scorer store (every cost kind, goal_mode); the priority a rotation by t % 3, which a floating segment leaves alone;
// the hidden layers a loop; the last layer-0 input xin, then x.
#define CEM_LEAN_TILE_TEMPLATE template <bool SEG>
#define CEM_LEAN_TILE cem_lean_tile
#define CEM_LEAN_HANDOVER_DECL const int wbk = 0; const __amdgpu_buffer_rsrc_t seg_rs = CEM_LEAN_SEG_RSRC();
#define CEM_LEAN_BKWAVE (w == wbk)
#define CEM_LEAN_HANDOVER seg_rs
#define CEM_LEAN_RING WRing wq; wq.init(p.wpack + (size_t)member_u * p.member_stride_f4 + p.wave_off_f4[w], lane, (int)p.wave_groups[w]);
#define CEM_LEAN_STAGE(KF, NOWN, L0IN, BASE) cem_lean_stage<KF, NOWN, L0IN>
#define CEM_LEAN_BOOKS_DECL \
    const int nk = 1 + p.sc.n_cost; \
    const float csz[4] = {p.sc.cost_size[0], p.sc.cost_size[1], p.sc.cost_size[2], p.sc.cost_size[3]}; \
    const float ind_cap = p.sc.indicator ? 1.0f : __builtin_inff(), clipv = p.sc.reward_clip > 0.f ? p.sc.reward_clip : __builtin_inff(); \
    const __amdgpu_buffer_rsrc_t cost_rs = __builtin_amdgcn_make_buffer_rsrc(p.costs, 0, p.costs ? (uint32_t)(H * p.Bloc) : 0u, 0x00020000);
#define CEM_LEAN_SCORE_D p.sc.D
#define CEM_LEAN_STORE_TERMS CEM_RARE_KINDS_AND_STORE(RC, NFW, p, part, w, q, j, nk, s, pm, tab_v, CEM_SEL0_LDS, tabl)
#define CEM_LEAN_PRIO_DECL \
    const bool prio_rot = !(SEG && tile_idx >= p.n_pinned); \
    const int prio_r0 = (tile_idx >> 8) % 3;
#define CEM_LEAN_PRIO_STEP \
    if (prio_rot) { \
        const int lvl = (t + prio_r0) % 3; \
        if (lvl == 0) __builtin_amdgcn_s_setprio(0); else if (lvl == 1) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(2); \
    }
#define CEM_LEAN_BOOKS_AT(T_) CEM_BOOKKEEP(p, td, part, w, wbk, lane, nk, csz, ind_cap, clipv, cost_rs, d_prev, c_prev, cum, done, T_);
#define CEM_LEAN_BOOKS_STEP if (!(resumed && first)) CEM_LEAN_BOOKS_AT(t - 1)
#define CEM_LEAN_BOOKS_END CEM_LEAN_BOOKS_AT(t_end - 1)
#define CEM_LEAN_HIDDEN_LAYERS _Pragma("unroll") for (int l = 1; l < 4; ++l) CEM_LEAN_HIDDEN(l + 1 < 4 ? l + 1 : 0, 0)
#define CEM_LEAN_HEADS (w < p.KB_obs)
#define CEM_LEAN_ISACT const f4 isact4 = CEM_TAB(tabl, CEM_ET_ACT, tv);
#define CEM_LEAN_NEXT_INPUT \
    f4 xin = sn; \
    if (wact) { \
        f4 act4; CEM_LEAN_ACTION(act4, e4, tn); \
        CEM_LEAN_KEEP(act4, t + 1); \
        xin = __builtin_elementwise_fma(isact4, act4, sn); \
    } \
    const f4 x = cem_sub4(xin, mn4) * rd4; \
    *reinterpret_cast<f4 *>(pub0 + xw) = x; \
    hB[0][0] = x;
#include "cem_rollout_lean_tile.h"
#undef CEM_LEAN_BOOKS_AT

}  // namespace

// one workgroup per tile, the whole horizon
__global__ __launch_bounds__(256) void cem_rollout_lean_kernel(const RolloutParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (p.check_done && p.ctrl->done) return;
    cem_lean_tile<false>(p, smem, (int)blockIdx.x, 0, p.H);
}

// Pinned tiles + floating segments: cem_rollout_seg_kernel's scheduler (CEM_SEG_SCHEDULE, cem_device.h) around the lean tile.
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
    CEM_SEG_SCHEDULE(p, item_s, tile, seg, t0, t1, (cem_lean_tile<true>(p, smem, tile, t0, t1)))
}

hipError_t launch_rollout_lean(const RolloutParams &p, int grid, hipStream_t st, bool seg)
{
    const size_t lds = CEM_LEAN_LDS_BYTES(p.H, (p.A + 3) / 4);
    if (seg) hipLaunchKernelGGL(cem_rollout_lean_seg_kernel, dim3(grid), dim3(256), lds, st, p);
    else hipLaunchKernelGGL(cem_rollout_lean_kernel, dim3(grid), dim3(256), lds, st, p);
    return hipGetLastError();
}
