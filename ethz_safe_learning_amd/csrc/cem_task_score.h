// cem_task_score.h — the task scorer (cem_planner_set_task): quadratic rewards and box state constraints for plans whose
// observation is no Safety-Gym lidar vector.  A task plan runs the handle's MODE 1 rollout kernel unchanged, with RolloutParams::traj
// pointed at a buffer the handle owns; ONE kernel, here, turns those trajectories and the candidates' actions into the `ret` and
// `costs` arrays the score, select, refit, keep and track kernels have always read (the rollout's own writes of the two are overwritten
// in stream order).  No rollout, sampler, reduce or select kernel changes, none reads what this one reads.
//
// THE CONTRACT (include/cem_mpc.h; planner.task_objective restates it in NumPy, bit for bit).  One row r of the rollout: states
// s_0 .. s_H raw and unscaled ([rows][H + 1][O], exactly what `traj` holds), actions a_0 .. a_{H-1} of candidate r mod N ([N][H][A]; the
// rows of a plan are p N + n, the reshape of mpc_policy.py:38).  Tables q, g, c, m, lo, hi [O] and rho [A]:
//   phi(s)  = sum_f [ q_f (s_f - g_f)^2 - c_f s_f ]
//   u(a)    = sum_j rho_j a_j^2
//   near(s) = R2 > 0 and sum_f m_f (s_f - g_f)^2 <= R2          R2 = fl32(goal_radius * goal_radius), rounded once on the host
//   viol(s) = 1.0 if any s_f < lo_f or s_f > hi_f, else 0.0      a NaN compares false
// and the bookkeeping of CEM_BOOKKEEP (cem_rollout_common.h), statement for statement, in both variant branches, with near(s_t) for
// `D_PREV <= goal_thresh`, -phi(s_{t+1}) - u(a_t) for `(D_PREV - dn) reward_distance` and viol(s_t) for C_PREV:
//   ga = near(s_t);  r = ((-phi(s_{t+1})) - u(a_t)) + (ga ? 1 : 0) * reward_goal;  r = fminf(fmaxf(r, -clip), clip)   (clip = +inf: none)
//   safe (safe_cem_mpc.py:86-93): done |= ga; nd = done ? 0 : 1; costs[t][r] = (uint8) (viol(s_t) * nd); cum += r * nd
//   cem  (mpc_policy.py:34-37):   nd = done ? 0 : 1; cum += r * nd; done |= ga            (no cost bytes)
// ret[r] = cum; a NaN is stored as the canonical quiet NaN 0x7fc00000 (a NaN's payload is no value: the host mirror stores the same).
//
// THE ARITHMETIC is fp32, every product and every sum rounded on its own (-ffp-contract=off), in ONE fixed order whatever the path:
//   per feature   d = s - g;  dd = d * d;  term = q * dd - c * s;  near term = m * dd
//   over features sixteen partial sums: partial l (0 .. 15) starts at +0 and adds the terms of features 64 i + 4 l + r, i = 0, 1 then
//                 r = 0 .. 3 (features >= O: tables q = c = m = 0 and s = g = 0, the term is +0); the sixteen are then added pairwise,
//                 neighbours first: (0 + 1), (2 + 3), ... then ((0 + 1) + (2 + 3)), ... four levels.  phi and the near sum alike.
//   over actions  u starts at +0 and adds rho_j * (a_j * a_j), j = 0 .. A - 1
//   over steps    t = 0 .. H - 1 as written above.
// The comparisons of near and viol are made on the ordered integer keys of the selects (cem_bits2key: the two zeros tie) behind a bit
// test for NaN, so -fno-honor-nans cannot change them.
//
// THE SHAPE.  The kernel is bound by the one read of `traj` (B2: 10 000 rows x 31 x 60 x 4 B = 74 MB): sixteen lanes own a row, lane l
// reads the feature quad 4 l (and 64 + 4 l on observations wider than 64) of one state with one 16-byte load — a state is O
// contiguous floats, the states of a row follow each other, so a 16-lane group walks its row's (H + 1) O floats front to back in
// pieces of up to 256 bytes and four rows share a wave.  CEM_TASK_DEPTH states are requested before the first is reduced (that many
// 16-byte loads per lane in flight).  Where a quad would not be 16-byte aligned (O % 4 != 0, or a caller's unaligned tensor) the same
// lanes read the same features element by element: same sums, same order.  The six tables sit in registers (6 x NT quads per lane,
// loaded once), rho in the kernel arguments.  No LDS, no atomics; the partial sums meet through four wave shuffles, the box test
// through one ballot.  Each word of `ret` and each cost byte is written once, by lane 0 of the row's group.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_score.hip defines
// CEM_TASK_SCORE_UNIT), as cem_plan_readout.h's is, so that the device code of cem_capi.hip stays what it was instruction for instruction.
#pragma once
#include "cem_device.h"
#include "../../include/cem_mpc.h"

#define CEM_TASK_THREADS 256
#define CEM_TASK_ROWS_PER_BLOCK (CEM_TASK_THREADS / 16)
#define CEM_TASK_DEPTH 4                 // states whose loads are in flight per lane
#define CEM_TASK_TABLES 6                // q, g, c, m, lo, hi: rows of TaskScoreParams::tab, CEM_U floats each
#define CEM_TASK_TAB_Q 0
#define CEM_TASK_TAB_G 1
#define CEM_TASK_TAB_C 2
#define CEM_TASK_TAB_M 3
#define CEM_TASK_TAB_LO 4
#define CEM_TASK_TAB_HI 5

struct TaskScoreParams {
    const float *traj;           // [rows][H + 1][O]
    const float *actions;        // [N][H][A]
    const float *tab;            // [CEM_TASK_TABLES][CEM_U], 16-byte aligned; beyond O: q = g = c = m = 0, lo = -inf, hi = +inf
    const CtrlBlock *ctrl;       // with check_done: a finished plan's launch returns at once (as the rollout in front of it did)
    float *ret;                  // [rows]
    uint8_t *costs;              // [H][rows] (variant 1), or null: no cost bytes
    int32_t rows, N, H, O, A, variant, check_done;
    float r2, reward_goal, clip; // fl32(goal_radius^2); clip = +inf: none
    float rho[CEM_MAX_ACT];
};

// Weak: a library built from cem_capi.hip alone has no task scorer and cem_planner_set_task says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_score(const TaskScoreParams &p, hipStream_t st);

#ifdef CEM_TASK_SCORE_UNIT
__device__ __forceinline__ bool cem_task_is_nan(const float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// NT: feature quads per lane (1: O <= 64, 2: O <= 128).  VEC: the quads are 16-byte aligned and whole (O % 4 == 0).
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_score_kernel(const TaskScoreParams p)
{
    if (p.check_done && p.ctrl->done) return;
    const int tid = (int)threadIdx.x, l = tid & 15, grp = (tid & 63) >> 4;
    const int row_raw = (int)blockIdx.x * CEM_TASK_ROWS_PER_BLOCK + (tid >> 4);
    const bool live = row_raw < p.rows;
    const int row = live ? row_raw : p.rows - 1;             // (a group past the end reads the last row and stores nothing: every lane reaches the shuffles)
    const int H = p.H, O = p.O, A = p.A;

    // this lane's quads of the six tables; lo / hi as the keys they are compared by
    f4 q4[NT], g4[NT], c4[NT], m4[NT];
    uint32_t klo[NT][4], khi[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int f0 = 64 * i + 4 * l;
        q4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_Q * CEM_U + f0);
        g4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_G * CEM_U + f0);
        c4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_C * CEM_U + f0);
        m4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_M * CEM_U + f0);
        const f4 lo = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_LO * CEM_U + f0);
        const f4 hi = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_HI * CEM_U + f0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { klo[i][r] = cem_f2key(lo[r]); khi[i][r] = cem_f2key(hi[r]); }
    }
    const uint32_t kr2 = cem_f2key(p.r2);
    const bool has_goal = !cem_task_is_nan(p.r2) && kr2 > cem_f2key(0.0f);

    const float *const tr = p.traj + (size_t)row * (size_t)(H + 1) * O;
    const float *const act = p.actions + (size_t)(row % p.N) * (size_t)H * A;

    float cum = 0.f;
    bool done = false, near_prev = false;
    float viol_prev = 0.f;
    for (int s0 = 0; s0 <= H; s0 += CEM_TASK_DEPTH) {
        // the loads of CEM_TASK_DEPTH states first (a step past the horizon reads the last state again and is not reduced)
        f4 x[CEM_TASK_DEPTH][NT];
#pragma unroll
        for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
            const int st = s0 + k <= H ? s0 + k : H;
            const float *const sp = tr + (size_t)st * O;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int f0 = 64 * i + 4 * l;
                if (VEC) x[k][i] = f0 < O ? *reinterpret_cast<const f4 *>(sp + f0) : f4{0.f, 0.f, 0.f, 0.f};
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[k][i][r] = f0 + r < O ? sp[f0 + r] : 0.f;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
            const int st = s0 + k;
            if (st > H) break;                               // (uniform: H is the launch's)
            float phi = 0.f, nsum = 0.f;
            bool out = false;
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = x[k][i][r];
                    const float d = s - g4[i][r];
                    const float dd = d * d;
                    phi = phi + (q4[i][r] * dd - c4[i][r] * s);
                    nsum = nsum + m4[i][r] * dd;
                    const uint32_t ks = cem_f2key(s);
                    out = out || (!cem_task_is_nan(s) && (ks < klo[i][r] || ks > khi[i][r]));
                }
            // the sixteen partial sums pairwise, neighbours first (an addition commutes: both lanes of a pair hold the same sum)
#pragma unroll
            for (int dl = 1; dl < 16; dl <<= 1) { phi = phi + __shfl_xor(phi, dl); nsum = nsum + __shfl_xor(nsum, dl); }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(out);
            const float viol = ((bal >> (16 * grp)) & 0xffffull) ? 1.0f : 0.0f;
            const bool near = has_goal && !cem_task_is_nan(nsum) && cem_f2key(nsum) <= kr2;
            if (st > 0) {
                const int t = st - 1;
                float u = 0.f;
                for (int j = 0; j < A; ++j) { const float a = act[(size_t)t * A + j]; u = u + p.rho[j] * (a * a); }
                const bool ga = near_prev;
                float r = ((-phi) - u) + (ga ? 1.0f : 0.0f) * p.reward_goal;
                r = fminf(fmaxf(r, -p.clip), p.clip);
                if (p.variant == 1) {                                                     /* safe_cem_mpc.py:86-93 */
                    done = done || ga;
                    const float nd = done ? 0.0f : 1.0f;
                    const float cst = viol_prev * nd;
                    if (p.costs && live && l == 0) p.costs[(size_t)t * p.rows + row] = (uint8_t)cst;
                    cum = cum + r * nd;
                } else {                                                                  /* mpc_policy.py:34-37 */
                    const float nd = done ? 0.0f : 1.0f;
                    cum = cum + r * nd;
                    done = done || ga;
                }
            }
            near_prev = near; viol_prev = viol;
        }
    }
    if (live && l == 0) reinterpret_cast<uint32_t *>(p.ret)[row] = cem_task_is_nan(cum) ? 0x7fc00000u : __float_as_uint(cum);
}

hipError_t launch_task_score(const TaskScoreParams &p, hipStream_t st)
{
    if (p.rows < 1 || p.N < 1 || p.H < 1 || p.O < 1 || p.O > CEM_U || p.A < 1 || p.A > CEM_MAX_ACT) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.rows + CEM_TASK_ROWS_PER_BLOCK - 1) / CEM_TASK_ROWS_PER_BLOCK)), block(CEM_TASK_THREADS);
    const bool vec = p.O % 4 == 0 && (reinterpret_cast<uintptr_t>(p.traj) & 15u) == 0;
    if (p.O <= 64) {
        if (vec) hipLaunchKernelGGL((cem_task_score_kernel<1, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_score_kernel<1, false>), grid, block, 0, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((cem_task_score_kernel<2, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_score_kernel<2, false>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}
#endif
