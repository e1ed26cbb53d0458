// cem_task_reference.h — the tracking task (cem_planner_set_task_tracking): the quadratic task of cem_task_score.h with a
// set-point that moves with time, a weight of its own on the last predicted state and a penalty on how fast the action changes.  A
// tracking plan launches what a quadratic-task plan launches, with ONE kernel, here, in the place of cem_task_score_kernel.
//
// THE CONTRACT (include/cem_mpc.h; planner.tracking_objective restates it in NumPy, bit for bit).  Everything not named here is
// cem_task_score.h's, statement for statement.  Tables q, c, m, lo, hi [O] and rho [A] as there; qT [O] (default q), kappa [A] (default
// 0), ref [T][O] with 1 <= T <= CEM_TASK_REF_MAX_STEPS; the clock (k0 >= 0, a_{-1} [A]).  For state s_st, st = 0 .. H:
//   j = min(k0 + st, T - 1)                       the reference row: the last row is held
//   d = s - ref[j];  dd = d * d;  term = w * dd - c * s  with w = qT where st == H, else q;  near term = m * dd
// the lane partials and the pairwise tree as there.  The action-rate term of step t starts at +0 and adds, j = 0 .. A - 1,
//   e = a_t[j] - a_{t-1}[j]  (a_{-1}: the clock's);  v = v + kappa_j * (e * e)          every operation rounded on its own
// and the reward is  r = (((-phi(s_{t+1})) - u(a_t)) - v_t) + (ga ? 1 : 0) * reward_goal;  the clip, the variant branches, the NaN
// canonicalisation and the key comparisons follow unchanged.  With T = 1, ref[0] = g, qT = q and kappa = 0 the result is
// cem_task_score_kernel's bit for bit (x - (+0) is x).
//
// THE SHAPE is cem_task_score_kernel's: sixteen lanes a row, lane l the feature quads 4 l (and 64 + 4 l), CEM_TASK_DEPTH states in
// flight, one or two quads per lane x 16-byte or element loads of the states.  The reference table is a device allocation of the
// handle's: row stride CEM_U floats, zero beyond O, 16-byte aligned — so a lane's reference quad is ONE 16-byte load whatever O is,
// requested with the state loads of the same batch (the table is a few KB to 8 MB: it stays in L2).  q, qT, c, m and the lo / hi keys sit
// in registers, rho and kappa in the kernel arguments.  k0 and a_{-1} are read from DEVICE MEMORY (the clock block: word 0 is k0, words
// 1 .. A are a_{-1}), never from the kernel arguments: a captured plan sees the clock that cem_planner_set_task_clock's stream-ordered
// copy left.  No LDS, no atomics.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_reference.hip defines
// CEM_TASK_REFERENCE_UNIT), as cem_task_score.h's is, so that every other unit's device code stays what it was instruction for instruction.
#pragma once
#include "cem_task_score.h"

#define CEM_TASK_REF_TAB_Q 0             // rows of TaskReferenceParams::tab: cem_task_score.h's, with qT where that has g
#define CEM_TASK_REF_TAB_QT 1
#define CEM_TASK_REF_TAB_C 2
#define CEM_TASK_REF_TAB_M 3
#define CEM_TASK_REF_TAB_LO 4
#define CEM_TASK_REF_TAB_HI 5
#define CEM_TASK_CLOCK_WORDS 64          // the clock block: k0 (int32), a_{-1} [CEM_MAX_ACT], padding

struct TaskReferenceParams {
    const float *traj;           // [rows][H + 1][O]
    const float *actions;        // [N][H][A]
    const float *tab;            // [CEM_TASK_TABLES][CEM_U], 16-byte aligned; beyond O: q = qT = c = m = 0, lo = -inf, hi = +inf
    const float *ref;            // [T][CEM_U], 16-byte aligned; zero beyond O
    const uint32_t *clock;       // [CEM_TASK_CLOCK_WORDS] in device memory: k0, then a_{-1} [A]
    const CtrlBlock *ctrl;       // with check_done: a finished plan's launch returns at once
    float *ret;                  // [rows]
    uint8_t *costs;              // [H][rows] (variant 1), or null: no cost bytes
    int32_t rows, N, H, O, A, variant, check_done, T;
    float r2, reward_goal, clip; // fl32(goal_radius^2); clip = +inf: none
    float rho[CEM_MAX_ACT], kappa[CEM_MAX_ACT];
};

// Weak: a library built without cem_task_reference.hip has no tracking task and cem_planner_set_task_tracking says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_reference(const TaskReferenceParams &p, hipStream_t st);

#ifdef CEM_TASK_REFERENCE_UNIT
__device__ __forceinline__ bool cem_task_ref_is_nan(const float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// NT: feature quads per lane (1: O <= 64, 2: O <= 128).  VEC: the state quads are 16-byte aligned and whole (O % 4 == 0).
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_reference_kernel(const TaskReferenceParams p)
{
    if (p.check_done && p.ctrl->done) return;
    const int tid = (int)threadIdx.x, l = tid & 15, grp = (tid & 63) >> 4;
    const int row_raw = (int)blockIdx.x * CEM_TASK_ROWS_PER_BLOCK + (tid >> 4);
    const bool live = row_raw < p.rows;
    const int row = live ? row_raw : p.rows - 1;             // (a group past the end reads the last row and stores nothing: every lane reaches the shuffles)
    const int H = p.H, O = p.O, A = p.A;

    // this lane's quads of the tables; lo / hi as the keys they are compared by
    f4 q4[NT], qT4[NT], c4[NT], m4[NT];
    uint32_t klo[NT][4], khi[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int f0 = 64 * i + 4 * l;
        q4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_Q * CEM_U + f0);
        qT4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_QT * CEM_U + f0);
        c4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_C * CEM_U + f0);
        m4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_M * CEM_U + f0);
        const f4 lo = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_LO * CEM_U + f0);
        const f4 hi = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_REF_TAB_HI * CEM_U + f0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { klo[i][r] = cem_f2key(lo[r]); khi[i][r] = cem_f2key(hi[r]); }
    }
    const uint32_t kr2 = cem_f2key(p.r2);
    const bool has_goal = !cem_task_ref_is_nan(p.r2) && kr2 > cem_f2key(0.0f);

    const float *const tr = p.traj + (size_t)row * (size_t)(H + 1) * O;
    const float *const act = p.actions + (size_t)(row % p.N) * (size_t)H * A;
    // the clock, from memory; the row of state st is min(k0 + st, T - 1) = min(min(k0, T - 1) + st, T - 1) (no overflow, and inside the
    // table whatever the word holds)
    const float *const aprev = reinterpret_cast<const float *>(p.clock + 1);
    const int last = p.T - 1;
    const int k0 = min(max((int)p.clock[0], 0), last);

    float cum = 0.f;
    bool done = false, near_prev = false;
    float viol_prev = 0.f;
    for (int s0 = 0; s0 <= H; s0 += CEM_TASK_DEPTH) {
        // the loads of CEM_TASK_DEPTH states and their reference rows first (a step past the horizon reads the last state again and is
        // not reduced)
        f4 x[CEM_TASK_DEPTH][NT], g[CEM_TASK_DEPTH][NT];
#pragma unroll
        for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
            const int st = s0 + k <= H ? s0 + k : H;
            const float *const sp = tr + (size_t)st * O;
            const float *const gp = p.ref + (size_t)min(k0 + st, last) * CEM_U;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int f0 = 64 * i + 4 * l;
                if (VEC) x[k][i] = f0 < O ? *reinterpret_cast<const f4 *>(sp + f0) : f4{0.f, 0.f, 0.f, 0.f};
                else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[k][i][r] = f0 + r < O ? sp[f0 + r] : 0.f;
                }
                g[k][i] = *reinterpret_cast<const f4 *>(gp + f0);
            }
        }
#pragma unroll
        for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
            const int st = s0 + k;
            if (st > H) break;                               // (uniform: H is the launch's)
            const bool terminal = st == H;
            float phi = 0.f, nsum = 0.f;
            bool out = false;
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = x[k][i][r];
                    const float d = s - g[k][i][r];
                    const float dd = d * d;
                    const float w = terminal ? qT4[i][r] : q4[i][r];
                    phi = phi + (w * dd - c4[i][r] * s);
                    nsum = nsum + m4[i][r] * dd;
                    const uint32_t ks = cem_f2key(s);
                    out = out || (!cem_task_ref_is_nan(s) && (ks < klo[i][r] || ks > khi[i][r]));
                }
            // the sixteen partial sums pairwise, neighbours first (an addition commutes: both lanes of a pair hold the same sum)
#pragma unroll
            for (int dl = 1; dl < 16; dl <<= 1) { phi = phi + __shfl_xor(phi, dl); nsum = nsum + __shfl_xor(nsum, dl); }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(out);
            const float viol = ((bal >> (16 * grp)) & 0xffffull) ? 1.0f : 0.0f;
            const bool near = has_goal && !cem_task_ref_is_nan(nsum) && cem_f2key(nsum) <= kr2;
            if (st > 0) {
                const int t = st - 1;
                const float *const at = act + (size_t)t * A;
                const float *const ap = t > 0 ? at - A : aprev;
                float u = 0.f, v = 0.f;
                for (int j = 0; j < A; ++j) {
                    const float a = at[j];
                    const float e = a - ap[j];
                    u = u + p.rho[j] * (a * a);
                    v = v + p.kappa[j] * (e * e);
                }
                const bool ga = near_prev;
                float r = (((-phi) - u) - v) + (ga ? 1.0f : 0.0f) * p.reward_goal;
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
    if (live && l == 0) reinterpret_cast<uint32_t *>(p.ret)[row] = cem_task_ref_is_nan(cum) ? 0x7fc00000u : __float_as_uint(cum);
}

hipError_t launch_task_reference(const TaskReferenceParams &p, hipStream_t st)
{
    if (p.rows < 1 || p.N < 1 || p.H < 1 || p.O < 1 || p.O > CEM_U || p.A < 1 || p.A > CEM_MAX_ACT || p.T < 1 || !p.ref || !p.clock) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.rows + CEM_TASK_ROWS_PER_BLOCK - 1) / CEM_TASK_ROWS_PER_BLOCK)), block(CEM_TASK_THREADS);
    const bool vec = p.O % 4 == 0 && (reinterpret_cast<uintptr_t>(p.traj) & 15u) == 0;
    if (p.O <= 64) {
        if (vec) hipLaunchKernelGGL((cem_task_reference_kernel<1, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_reference_kernel<1, false>), grid, block, 0, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((cem_task_reference_kernel<2, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_reference_kernel<2, false>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}
#endif
