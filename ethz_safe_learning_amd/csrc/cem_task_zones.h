// cem_task_zones.h — keep-out and keep-in zones on a task (cem_planner_set_task_zones): up to CEM_TASK_MAX_ZONES
// axis-aligned ellipsoids on up to CEM_TASK_ZONE_AXES state features each, which a plan must stay out of (hazards, pillars) or inside
// of.  A zone that is hit sets the step's cost byte exactly as the box does; a zone that is near costs reward through a hinge.  A task
// plan with zones launches what its base task plan launches, with ONE kernel, here, in the place of cem_task_score_kernel /
// cem_task_reference_kernel.  A task without zones never comes here.
//
// THE CONTRACT (include/cem_mpc.h; planner.task_objective / tracking_objective restate it in NumPy, bit for bit).  Everything not named
// here is cem_task_reference.h's, statement for statement; a quadratic base task is the tracking task with one reference row g, qT = q,
// kappa = 0 and the clock at (0, zeros).  Zone z: axes axis[z][d] (-1: slot unused), centre c[z][d], weights w[z][d], R2 = fl32(radius^2),
// Rm2 = fl32((radius + margin)^2) (keep-in: (radius - margin)^2), both rounded once on the host, penalty, keep_in.  For state s:
//   dist2 starts at +0; d = 0 .. 3 with a used axis:  e = s[axis] - c;  dist2 = dist2 + w * (e * e)      every operation rounded on its own
//   keep-out: hit = dist2 <= R2;  hinge = fmaxf(Rm2 - dist2, 0)        keep-in: hit = dist2 > R2;  hinge = fmaxf(dist2 - Rm2, 0)
//   a NaN dist2 hits nothing and its hinge is +0; the comparisons are made on the selects' integer keys behind the NaN bit test
//   pen(s): sixteen slots, slot z = penalty_z * hinge_z (z >= n_zones: +0), added pairwise, neighbours first, four levels
//   viol(s) = the box's viol(s) or any hit_z(s)
//   r = ((((-phi(s_{t+1})) - u(a_t)) - v_t) - pen(s_{t+1})) + (ga ? 1 : 0) * reward_goal;  the clip and the variant branches unchanged.
//
// THE SHAPE is cem_task_reference_kernel's, and the sixteen lanes that own a row own one zone each: lane l evaluates zone l on the
// state its group has just loaded.  Its <= 4 axis features are element loads of the same state, requested in the same batch as the
// state's quads (they hit the lines those fetch: no second read of `traj` from memory).  `hit` joins the box test in front of the one
// ballot, `pen` goes through the four shuffles phi and the near sum go through.  The zone table is a device allocation of the handle's,
// sixteen words a zone (CEM_TASK_ZONE_WORDS): a lane reads its zone's four 16-byte rows once, in front of the loop.  No LDS, no atomics.
//
// This header is what cem_capi.hip includes; the kernel is compiled in a translation unit of its own (cem_task_zones.hip defines
// CEM_TASK_ZONES_UNIT), so that every other unit's device code stays what it was instruction for instruction.
#pragma once
#include "cem_task_reference.h"

#define CEM_TASK_ZONE_WORDS 16           // a zone in the device table: axis [4] (int32), centre [4], weight [4], R2, Rm2, penalty, keep_in (int32)
#define CEM_TASK_ZONE_ROW_AXIS 0
#define CEM_TASK_ZONE_ROW_CENTRE 4
#define CEM_TASK_ZONE_ROW_WEIGHT 8
#define CEM_TASK_ZONE_R2 12
#define CEM_TASK_ZONE_RM2 13
#define CEM_TASK_ZONE_PENALTY 14
#define CEM_TASK_ZONE_KEEP_IN 15

struct TaskZonesParams {
    const float *traj;           // [rows][H + 1][O]
    const float *actions;        // [N][H][A]
    const float *tab;            // cem_task_reference.h's: [CEM_TASK_TABLES][CEM_U] with qT in the second row
    const float *ref;            // [T][CEM_U], 16-byte aligned; zero beyond O (a quadratic base: one row, g)
    const uint32_t *clock;       // [CEM_TASK_CLOCK_WORDS] in device memory (a quadratic base: zeros)
    const uint32_t *zones;       // [CEM_TASK_MAX_ZONES][CEM_TASK_ZONE_WORDS], 16-byte aligned; zones >= n_zones: no axis, penalty +0
    const CtrlBlock *ctrl;       // with check_done: a finished plan's launch returns at once
    float *ret;                  // [rows]
    uint8_t *costs;              // [H][rows] (variant 1), or null: no cost bytes
    int32_t rows, N, H, O, A, variant, check_done, T, n_zones;
    float r2, reward_goal, clip; // fl32(goal_radius^2); clip = +inf: none
    float rho[CEM_MAX_ACT], kappa[CEM_MAX_ACT];
};

// Weak: a library built without cem_task_zones.hip has no zones and cem_planner_set_task_zones says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_task_zones(const TaskZonesParams &p, hipStream_t st);

#ifdef CEM_TASK_ZONES_UNIT
typedef uint32_t cem_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool cem_task_zone_is_nan(const float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }

// NT: feature quads per lane (1: O <= 64, 2: O <= 128).  VEC: the state quads are 16-byte aligned and whole (O % 4 == 0).
template <int NT, bool VEC>
__global__ __launch_bounds__(CEM_TASK_THREADS) void cem_task_zones_kernel(const TaskZonesParams p)
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
    const bool has_goal = !cem_task_zone_is_nan(p.r2) && kr2 > cem_f2key(0.0f);

    // this lane's zone: four 16-byte rows of the table.  A slot is used where its axis names a feature of the state (the setter
    // refuses any other axis but -1; the test here keeps a load inside the state whatever the table holds)
    const uint32_t *const zp = p.zones + (size_t)l * CEM_TASK_ZONE_WORDS;
    const cem_u4 zax = *reinterpret_cast<const cem_u4 *>(zp + CEM_TASK_ZONE_ROW_AXIS);
    const f4 zc = *reinterpret_cast<const f4 *>(zp + CEM_TASK_ZONE_ROW_CENTRE);
    const f4 zw = *reinterpret_cast<const f4 *>(zp + CEM_TASK_ZONE_ROW_WEIGHT);
    const cem_u4 zr = *reinterpret_cast<const cem_u4 *>(zp + CEM_TASK_ZONE_R2);
    const bool zone_on = l < p.n_zones;
    bool zused[CEM_TASK_ZONE_AXES];
    int zoff[CEM_TASK_ZONE_AXES];
#pragma unroll
    for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) { zused[d] = zone_on && zax[d] < (uint32_t)O; zoff[d] = zused[d] ? (int)zax[d] : 0; }
    const uint32_t kR2 = cem_f2key(__uint_as_float(zr[0]));
    const float zRm2 = __uint_as_float(zr[1]), zpen = __uint_as_float(zr[2]);
    const bool keep_in = zr[3] != 0u;

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
        // the loads of CEM_TASK_DEPTH states, their reference rows and this lane's zone features first (a step past the horizon reads
        // the last state again and is not reduced)
        f4 x[CEM_TASK_DEPTH][NT], g[CEM_TASK_DEPTH][NT];
        float zs[CEM_TASK_DEPTH][CEM_TASK_ZONE_AXES];
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
#pragma unroll
            for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) zs[k][d] = sp[zoff[d]];     // (an unused slot reads feature 0 and drops it)
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
                    out = out || (!cem_task_zone_is_nan(s) && (ks < klo[i][r] || ks > khi[i][r]));
                }
            // this lane's zone on the same state
            float dist2 = 0.f;
#pragma unroll
            for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) {
                const float e = zs[k][d] - zc[d];
                const float with = dist2 + zw[d] * (e * e);
                dist2 = zused[d] ? with : dist2;
            }
            const bool dnan = cem_task_zone_is_nan(dist2);
            const uint32_t kd = cem_f2key(dist2);
            const bool inside = kd <= kR2;
            const bool hit = zone_on && !dnan && (keep_in ? !inside : inside);
            const float gap = keep_in ? dist2 - zRm2 : zRm2 - dist2;
            // (gap is no NaN behind the bit test, and an exact difference of zero is +0: the larger of gap and +0, by its key)
            const float hinge = (!dnan && !cem_task_zone_is_nan(gap) && cem_f2key(gap) > cem_f2key(0.0f)) ? gap : 0.0f;
            float pen = zone_on ? zpen * hinge : 0.0f;
            out = out || hit;
            // the sixteen partial sums pairwise, neighbours first (an addition commutes: both lanes of a pair hold the same sum)
#pragma unroll
            for (int dl = 1; dl < 16; dl <<= 1) { phi = phi + __shfl_xor(phi, dl); nsum = nsum + __shfl_xor(nsum, dl); pen = pen + __shfl_xor(pen, dl); }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(out);
            const float viol = ((bal >> (16 * grp)) & 0xffffull) ? 1.0f : 0.0f;
            const bool near = has_goal && !cem_task_zone_is_nan(nsum) && cem_f2key(nsum) <= kr2;
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
                float r = ((((-phi) - u) - v) - pen) + (ga ? 1.0f : 0.0f) * p.reward_goal;
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
    if (live && l == 0) reinterpret_cast<uint32_t *>(p.ret)[row] = cem_task_zone_is_nan(cum) ? 0x7fc00000u : __float_as_uint(cum);
}

hipError_t launch_task_zones(const TaskZonesParams &p, hipStream_t st)
{
    if (p.rows < 1 || p.N < 1 || p.H < 1 || p.O < 1 || p.O > CEM_U || p.A < 1 || p.A > CEM_MAX_ACT || p.T < 1 || !p.ref || !p.clock || !p.zones ||
        p.n_zones < 1 || p.n_zones > CEM_TASK_MAX_ZONES) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.rows + CEM_TASK_ROWS_PER_BLOCK - 1) / CEM_TASK_ROWS_PER_BLOCK)), block(CEM_TASK_THREADS);
    const bool vec = p.O % 4 == 0 && (reinterpret_cast<uintptr_t>(p.traj) & 15u) == 0;
    if (p.O <= 64) {
        if (vec) hipLaunchKernelGGL((cem_task_zones_kernel<1, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_zones_kernel<1, false>), grid, block, 0, st, p);
    } else {
        if (vec) hipLaunchKernelGGL((cem_task_zones_kernel<2, true>), grid, block, 0, st, p);
        else hipLaunchKernelGGL((cem_task_zones_kernel<2, false>), grid, block, 0, st, p);
    }
    return hipGetLastError();
}
#endif
