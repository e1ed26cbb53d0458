// cem_task_tile.h — the ONE task-scoring tile: what cem_task_score_kernel, cem_task_reference_kernel,
// cem_task_zones_kernel and cem_task_outputs_kernel share, which is everything but a few statements each.  The four headers of those
// names hold their contracts, their weak launchers and a wrapper of one line; cem_capi.hip includes them, and each kernel is compiled
// in a unit of its own.
//
// THE KINDS.  cem_task_rows<NT, VEC, KIND> is the body of all four; `if constexpr` on KIND keeps each kind's statements exactly what
// its header states, in that order and with those parentheses (-ffp-contract=off: no statement is re-associated across kinds):
//   CEM_TASK_KIND_QUADRATIC  g from row CEM_TASK_TAB_G of the tables;  r = ((-phi) - u) + ...
//   CEM_TASK_KIND_TRACKING   g from `ref` at the clock's row, qT (the same table row) on the terminal state, v from kappa;  ... - v
//   CEM_TASK_KIND_ZONES      tracking, and lane l's zone on every state: `hit` joins the ballot, `pen` the shuffles;  ... - pen
//   CEM_TASK_KIND_OUTPUTS    zones (n_zones may be 0), and lane l's linear output y_l = C[l] . s of every state: its terms join lane l's
//                            partial sums, its bounds the ballot, and a zone axis may name it (cem_task_outputs.h).  The one kind with LDS: C
// A later kind is a superset of the one before it (KIND >= ... below).  TaskParams is the superset's parameter block; a kind reads
// only its own fields (the launcher's checks are per kind too).
//
// THE SHAPE.  The kernels are bound by the one read of `traj` (B2: 10 000 rows x 31 x 60 x 4 B = 74 MB): sixteen lanes own a row, lane l
// reads the feature quad 4 l (and 64 + 4 l on observations wider than 64) of one state with one 16-byte load — a state is O
// contiguous floats, the states of a row follow each other, so a 16-lane group walks its row's (H + 1) O floats front to back in
// pieces of up to 256 bytes and four rows share a wave.  CEM_TASK_DEPTH states are requested before the first is reduced (that many
// 16-byte loads per lane in flight); a tracking kind requests their reference quads, a zoned one its lane's <= 4 axis features, in
// the same batch.  Where a quad would not be 16-byte aligned (O % 4 != 0, or a caller's unaligned tensor) the same lanes read the same
// features element by element: same sums, same order.  The tables sit in registers (6 x NT quads per lane, loaded once), rho and
// kappa in the kernel arguments, the clock in device memory.  No LDS (but the outputs kind's C), no atomics; the partial sums meet through four wave shuffles,
// the box test (and the zones' hits) through one ballot.  A group past the end reads the last row and stores nothing: every lane
// reaches the shuffles.  Each word of `ret` and each cost byte is written once, by lane 0 of the row's group.
#pragma once
#include "cem_device.h"
#include "../../include/cem_mpc.h"

#define CEM_TASK_THREADS 256
#define CEM_TASK_ROWS_PER_BLOCK (CEM_TASK_THREADS / 16)
#define CEM_TASK_DEPTH 4                 // states whose loads are in flight per lane
#define CEM_TASK_TABLES 6                // rows of TaskParams::tab, CEM_U floats each: q, g (quadratic) or qT (tracking), c, m, lo, hi
#define CEM_TASK_TAB_Q 0
#define CEM_TASK_TAB_G 1
#define CEM_TASK_TAB_QT 1
#define CEM_TASK_TAB_C 2
#define CEM_TASK_TAB_M 3
#define CEM_TASK_TAB_LO 4
#define CEM_TASK_TAB_HI 5
#define CEM_TASK_CLOCK_WORDS 64          // the clock block: k0 (int32), a_{-1} [CEM_MAX_ACT], padding
#define CEM_TASK_ZONE_WORDS 16           // a zone in the device table: axis [4] (int32), centre [4], weight [4], R2, Rm2, penalty, keep_in (int32)
#define CEM_TASK_ZONE_ROW_AXIS 0
#define CEM_TASK_ZONE_ROW_CENTRE 4
#define CEM_TASK_ZONE_ROW_WEIGHT 8
#define CEM_TASK_ZONE_R2 12
#define CEM_TASK_ZONE_RM2 13
#define CEM_TASK_ZONE_PENALTY 14
#define CEM_TASK_ZONE_KEEP_IN 15

#define CEM_TASK_KIND_QUADRATIC 0
#define CEM_TASK_KIND_TRACKING 1
#define CEM_TASK_KIND_ZONES 2
#define CEM_TASK_KIND_OUTPUTS 3
#define CEM_TASK_OUT_TABLES 6            // rows of TaskParams::out_tab, CEM_TASK_MAX_OUTPUTS floats each: qy, qTy, cy, my, loy, hiy (outputs >= n_outputs: 0, 0, 0, 0, -inf, +inf)
#define CEM_TASK_OUT_TAB_Q 0
#define CEM_TASK_OUT_TAB_QT 1
#define CEM_TASK_OUT_TAB_C 2
#define CEM_TASK_OUT_TAB_M 3
#define CEM_TASK_OUT_TAB_LO 4
#define CEM_TASK_OUT_TAB_HI 5

struct TaskParams {
    const float *traj;           // [rows][H + 1][O]
    const float *actions;        // [N][H][A]
    const float *tab;            // [CEM_TASK_TABLES][CEM_U], 16-byte aligned; beyond O: q = g = qT = c = m = 0, lo = -inf, hi = +inf
    const float *ref;            // tracking: [T][CEM_U], 16-byte aligned; zero beyond O (zones on a quadratic base: one row, g)
    const uint32_t *clock;       // tracking: [CEM_TASK_CLOCK_WORDS] in device memory: k0, then a_{-1} [A] (zones on a quadratic base: zeros)
    const uint32_t *zones;       // zones: [CEM_TASK_MAX_ZONES][CEM_TASK_ZONE_WORDS], 16-byte aligned; zones >= n_zones: no axis, penalty +0
    const CtrlBlock *ctrl;       // with check_done: a finished plan's launch returns at once (as the rollout in front of it did)
    float *ret;                  // [rows]
    uint8_t *costs;              // [H][rows] (variant 1), or null: no cost bytes
    int32_t rows, N, H, O, A, variant, check_done, T, n_zones;
    float r2, reward_goal, clip; // fl32(goal_radius^2); clip = +inf: none
    float rho[CEM_MAX_ACT], kappa[CEM_MAX_ACT];
    // outputs (cem_task_outputs.h), read by CEM_TASK_KIND_OUTPUTS alone
    const float *out_c;          // [CEM_TASK_MAX_OUTPUTS][CEM_U], 16-byte aligned; zero beyond O and from row n_outputs on
    const float *out_tab;        // [CEM_TASK_OUT_TABLES][CEM_TASK_MAX_OUTPUTS]
    const float *out_ref;        // [out_T][CEM_TASK_MAX_OUTPUTS]: the outputs' targets, one row or the base task's T rows (the same clock)
    int32_t n_outputs, out_T;
};

#if defined(CEM_TASK_SCORE_UNIT) || defined(CEM_TASK_REFERENCE_UNIT) || defined(CEM_TASK_ZONES_UNIT) || defined(CEM_TASK_OUTPUTS_UNIT)
typedef uint32_t cem_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bool cem_task_is_nan(const float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
// The outputs kind's lane predicates would not fit beside the zones kind's in the scalar file: it keeps them as masks in vector registers.
// cem_task_mask: all ones where the condition holds (through an empty asm, or the compiler folds mask and pick back into a select on a
// scalar register pair); cem_task_pick: a where the lane's mask is all ones, b where it is zero — the same bits a select gives
__device__ __forceinline__ uint32_t cem_task_mask(const bool on) { uint32_t m = on ? 0xffffffffu : 0u; asm volatile("" : "+v"(m)); return m; }
__device__ __forceinline__ float cem_task_pick(const uint32_t mask, const float a, const float b) { return __uint_as_float((__float_as_uint(a) & mask) | (__float_as_uint(b) & ~mask)); }

// NT: feature quads per lane (1: O <= 64, 2: O <= 128).  VEC: the state quads are 16-byte aligned and whole (O % 4 == 0).
template <int NT, bool VEC, int KIND>
__device__ __forceinline__ void cem_task_rows(const TaskParams &p)
{
    constexpr bool TRACK = KIND >= CEM_TASK_KIND_TRACKING, ZONED = KIND >= CEM_TASK_KIND_ZONES, OUTS = KIND >= CEM_TASK_KIND_OUTPUTS;
    if (p.check_done && p.ctrl->done) return;
    const int tid = (int)threadIdx.x, l = tid & 15, grp = (tid & 63) >> 4;
    // outputs: C in LDS, 8 KB, copied once by the whole block (the return above is the block's as a whole); lane l's own tables in registers
    float *cl = nullptr;
    uint32_t out_on = 0u;                    // (all ones: this lane owns an output)
    float qy = 0.f, qTy = 0.f, cy = 0.f, my = 0.f;
    uint32_t kloy = 0u, khiy = 0u;
    int gy_stride = 0;                       // floats between the rows of out_ref that two reference rows of the base task read: 0 where it has one row
    if constexpr (OUTS) {
        __shared__ f4 c_lds[CEM_TASK_MAX_OUTPUTS * CEM_U / 4];
#pragma unroll
        for (int j = 0; j < CEM_TASK_MAX_OUTPUTS * CEM_U / 4 / CEM_TASK_THREADS; ++j)
            c_lds[j * CEM_TASK_THREADS + tid] = reinterpret_cast<const f4 *>(p.out_c)[j * CEM_TASK_THREADS + tid];
        __syncthreads();
        cl = reinterpret_cast<float *>(c_lds);
        out_on = cem_task_mask(l < p.n_outputs);
        gy_stride = p.out_T > 1 ? CEM_TASK_MAX_OUTPUTS : 0;
        qy = p.out_tab[CEM_TASK_OUT_TAB_Q * CEM_TASK_MAX_OUTPUTS + l]; qTy = p.out_tab[CEM_TASK_OUT_TAB_QT * CEM_TASK_MAX_OUTPUTS + l];
        cy = p.out_tab[CEM_TASK_OUT_TAB_C * CEM_TASK_MAX_OUTPUTS + l]; my = p.out_tab[CEM_TASK_OUT_TAB_M * CEM_TASK_MAX_OUTPUTS + l];
        kloy = cem_f2key(p.out_tab[CEM_TASK_OUT_TAB_LO * CEM_TASK_MAX_OUTPUTS + l]); khiy = cem_f2key(p.out_tab[CEM_TASK_OUT_TAB_HI * CEM_TASK_MAX_OUTPUTS + l]);
    }
    const int row_raw = (int)blockIdx.x * CEM_TASK_ROWS_PER_BLOCK + (tid >> 4);
    const bool live = row_raw < p.rows;
    const int row = live ? row_raw : p.rows - 1;             // (a group past the end reads the last row and stores nothing: every lane reaches the shuffles)
    const int H = p.H, O = p.O, A = p.A;

    // this lane's quads of the six tables (gT4: g of a quadratic task, qT of a tracking one); lo / hi as the keys they are compared by
    f4 q4[NT], gT4[NT], c4[NT], m4[NT];
    uint32_t klo[NT][4], khi[NT][4];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        const int f0 = 64 * i + 4 * l;
        q4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_Q * CEM_U + f0);
        gT4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_G * CEM_U + f0);
        c4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_C * CEM_U + f0);
        m4[i] = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_M * CEM_U + f0);
        const f4 lo = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_LO * CEM_U + f0);
        const f4 hi = *reinterpret_cast<const f4 *>(p.tab + CEM_TASK_TAB_HI * CEM_U + f0);
#pragma unroll
        for (int r = 0; r < 4; ++r) { klo[i][r] = cem_f2key(lo[r]); khi[i][r] = cem_f2key(hi[r]); }
    }
    const uint32_t kr2 = cem_f2key(p.r2);
    const bool has_goal = !cem_task_is_nan(p.r2) && kr2 > cem_f2key(0.0f);

    // zones: this lane's zone, four 16-byte rows of the table.  A slot is used where its axis names a feature of the state (the setter
    // refuses any other axis but -1; the test here keeps a load inside the state whatever the table holds)
    f4 zc = {0.f, 0.f, 0.f, 0.f}, zw = zc;
    bool zone_on = false, keep_in = false, zused[CEM_TASK_ZONE_AXES] = {};
    int zoff[CEM_TASK_ZONE_AXES] = {};
    uint32_t zout[CEM_TASK_ZONE_AXES] = {};  // outputs: all ones where the axis names output zsrc - (this group's first lane), held by that lane
    int zsrc[CEM_TASK_ZONE_AXES] = {};
    uint32_t zusedm[CEM_TASK_ZONE_AXES] = {}, zonem = 0u, keepm = 0u;   // outputs: zused, zone_on and keep_in as masks in vector registers (cem_task_pick)
    uint32_t kR2 = 0u;
    float zRm2 = 0.f, zpen = 0.f;
    if constexpr (ZONED) {
        const uint32_t *const zp = p.zones + (size_t)l * CEM_TASK_ZONE_WORDS;
        const cem_u4 zax = *reinterpret_cast<const cem_u4 *>(zp + CEM_TASK_ZONE_ROW_AXIS);
        zc = *reinterpret_cast<const f4 *>(zp + CEM_TASK_ZONE_ROW_CENTRE);
        zw = *reinterpret_cast<const f4 *>(zp + CEM_TASK_ZONE_ROW_WEIGHT);
        const cem_u4 zr = *reinterpret_cast<const cem_u4 *>(zp + CEM_TASK_ZONE_R2);
        zone_on = l < p.n_zones;
#pragma unroll
        for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) {
            const bool feat = zone_on && zax[d] < (uint32_t)O;
            if constexpr (OUTS) {
                const bool named = zone_on && !feat && zax[d] - (uint32_t)O < (uint32_t)p.n_outputs;
                zout[d] = cem_task_mask(named);
                zsrc[d] = (tid & 48) | (named ? (int)(zax[d] - (uint32_t)O) : 0);
                zused[d] = feat || named; zusedm[d] = cem_task_mask(zused[d]);
            } else zused[d] = feat;
            zoff[d] = feat ? (int)zax[d] : 0;
        }
        kR2 = cem_f2key(__uint_as_float(zr[0]));
        zRm2 = __uint_as_float(zr[1]); zpen = __uint_as_float(zr[2]);
        keep_in = zr[3] != 0u;
        if constexpr (OUTS) { zonem = cem_task_mask(zone_on); keepm = cem_task_mask(keep_in); }
    }

    const float *const tr = p.traj + (size_t)row * (size_t)(H + 1) * O;
    const float *const act = p.actions + (size_t)(row % p.N) * (size_t)H * A;
    // tracking: the clock, from memory; the row of state st is min(k0 + st, T - 1) = min(min(k0, T - 1) + st, T - 1) (no overflow, and
    // inside the table whatever the word holds)
    const float *aprev = nullptr;
    int last = 0, k0 = 0;
    if constexpr (TRACK) {
        aprev = reinterpret_cast<const float *>(p.clock + 1);
        last = p.T - 1;
        k0 = min(max((int)p.clock[0], 0), last);
    }

    float cum = 0.f;
    bool done = false, near_prev = false;
    float viol_prev = 0.f;
    for (int s0 = 0; s0 <= H; s0 += CEM_TASK_DEPTH) {
        // the loads of CEM_TASK_DEPTH states first, with their reference rows and this lane's zone features where the kind has them (a
        // step past the horizon reads the last state again and is not reduced)
        f4 x[CEM_TASK_DEPTH][NT], g[CEM_TASK_DEPTH][NT];
        float zs[CEM_TASK_DEPTH][CEM_TASK_ZONE_AXES], gy[CEM_TASK_DEPTH] = {};
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
                if constexpr (TRACK) g[k][i] = *reinterpret_cast<const f4 *>(p.ref + (size_t)min(k0 + st, last) * CEM_U + f0);
                else g[k][i] = gT4[i];
            }
            if constexpr (ZONED) {
#pragma unroll
                for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) zs[k][d] = sp[zoff[d]];     // (an unused slot reads feature 0 and drops it)
            }
            if constexpr (OUTS) gy[k] = p.out_ref[(size_t)min(k0 + st, last) * gy_stride + l];    // (out_T is T or 1, the launcher's check: inside the table)
        }
        // outputs: this lane's sixteen partial dot products of every state in flight (a row of C is read once for all of them; a row from
        // n_outputs on is skipped, uniformly — on a count the compiler cannot see through, or it would keep the sixteen conditions in
        // scalar registers across the loop and spill), then the butterfly: at distance dl a lane keeps the outputs whose bit dl is its own and
        // adds its partner's partials of those, so that lane l ends with y_l, the sixteen partials added pairwise, neighbours first
        float y[CEM_TASK_DEPTH] = {};
        if constexpr (OUTS) {
            float yp[CEM_TASK_DEPTH][CEM_TASK_MAX_OUTPUTS];
            int n_out = p.n_outputs;
            asm volatile("" : "+s"(n_out));
#pragma unroll
            for (int m = 0; m < CEM_TASK_MAX_OUTPUTS; ++m) {
                if (m < n_out) {
                    f4 cq[NT];
#pragma unroll
                    for (int i = 0; i < NT; ++i) cq[i] = *reinterpret_cast<const f4 *>(cl + m * CEM_U + 64 * i + 4 * l);
#pragma unroll
                    for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
                        float a = 0.f;
#pragma unroll
                        for (int i = 0; i < NT; ++i)
#pragma unroll
                            for (int r = 0; r < 4; ++r) a = a + cq[i][r] * x[k][i][r];
                        yp[k][m] = a;
                    }
                } else {
#pragma unroll
                    for (int k = 0; k < CEM_TASK_DEPTH; ++k) yp[k][m] = 0.f;
                }
            }
#pragma unroll
            for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
                float a8[8], a4[4], a2[2];
                const uint32_t b0 = 0u - (uint32_t)(l & 1), b1 = 0u - (uint32_t)((l >> 1) & 1), b2 = 0u - (uint32_t)((l >> 2) & 1), b3 = 0u - (uint32_t)((l >> 3) & 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) a8[j] = cem_task_pick(b0, yp[k][2 * j + 1], yp[k][2 * j]) + __shfl_xor(cem_task_pick(b0, yp[k][2 * j], yp[k][2 * j + 1]), 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) a4[j] = cem_task_pick(b1, a8[2 * j + 1], a8[2 * j]) + __shfl_xor(cem_task_pick(b1, a8[2 * j], a8[2 * j + 1]), 2);
#pragma unroll
                for (int j = 0; j < 2; ++j) a2[j] = cem_task_pick(b2, a4[2 * j + 1], a4[2 * j]) + __shfl_xor(cem_task_pick(b2, a4[2 * j], a4[2 * j + 1]), 4);
                y[k] = cem_task_pick(b3, a2[1], a2[0]) + __shfl_xor(cem_task_pick(b3, a2[0], a2[1]), 8);
            }
        }
#pragma unroll
        for (int k = 0; k < CEM_TASK_DEPTH; ++k) {
            const int st = s0 + k;
            if (st > H) break;                               // (uniform: H is the launch's)
            const bool terminal = TRACK && st == H;
            float phi = 0.f, nsum = 0.f, pen = 0.f;
            bool out = false;
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float s = x[k][i][r];
                    const float d = s - g[k][i][r];
                    const float dd = d * d;
                    const float w = terminal ? gT4[i][r] : q4[i][r];
                    phi = phi + (w * dd - c4[i][r] * s);
                    nsum = nsum + m4[i][r] * dd;
                    const uint32_t ks = cem_f2key(s);
                    out = out || (!cem_task_is_nan(s) && (ks < klo[i][r] || ks > khi[i][r]));
                }
            if constexpr (OUTS) {
                // this lane's output on the same state: its terms behind the lane's feature terms, its bounds with the box's
                const float yv = y[k];
                const float e = yv - gy[k];
                const float ee = e * e;
                const float w = terminal ? qTy : qy;
                const float withphi = phi + (w * ee - cy * yv), withn = nsum + my * ee;
                phi = cem_task_pick(out_on, withphi, phi); nsum = cem_task_pick(out_on, withn, nsum);
                const uint32_t ky = cem_f2key(yv);
                out = out || (!cem_task_is_nan(yv) && (ky < kloy || ky > khiy));            // (a lane without an output holds infinite bounds)
            }
            if constexpr (ZONED) {
                // this lane's zone on the same state
                float dist2 = 0.f;
#pragma unroll
                for (int d = 0; d < CEM_TASK_ZONE_AXES; ++d) {
                    if constexpr (OUTS) { const float yz = __shfl(y[k], zsrc[d]); zs[k][d] = cem_task_pick(zout[d], yz, zs[k][d]); }   // (every lane reads: one variable-source lane read)
                    const float e = zs[k][d] - zc[d];
                    const float with = dist2 + zw[d] * (e * e);
                    if constexpr (OUTS) dist2 = cem_task_pick(zusedm[d], with, dist2);
                    else dist2 = zused[d] ? with : dist2;
                }
                const bool dnan = cem_task_is_nan(dist2);
                const uint32_t kd = cem_f2key(dist2);
                const bool inside = kd <= kR2;
                bool hit;
                float gap;
                if constexpr (OUTS) {                                                     // (the same values, selected by the masks)
                    hit = ((((inside ? 0xffffffffu : 0u) ^ keepm) & zonem) != 0u) && !dnan;
                    gap = cem_task_pick(keepm, dist2 - zRm2, zRm2 - dist2);
                } else {
                    hit = zone_on && !dnan && (keep_in ? !inside : inside);
                    gap = keep_in ? dist2 - zRm2 : zRm2 - dist2;
                }
                // (gap is no NaN behind the bit test, and an exact difference of zero is +0: the larger of gap and +0, by its key)
                const float hinge = (!dnan && !cem_task_is_nan(gap) && cem_f2key(gap) > cem_f2key(0.0f)) ? gap : 0.0f;
                if constexpr (OUTS) pen = cem_task_pick(zonem, zpen * hinge, 0.0f);
                else pen = zone_on ? zpen * hinge : 0.0f;
                out = out || hit;
            }
            // the sixteen partial sums pairwise, neighbours first (an addition commutes: both lanes of a pair hold the same sum)
#pragma unroll
            for (int dl = 1; dl < 16; dl <<= 1) {
                phi = phi + __shfl_xor(phi, dl); nsum = nsum + __shfl_xor(nsum, dl);
                if constexpr (ZONED) pen = pen + __shfl_xor(pen, dl);
            }
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(out);
            const float viol = ((bal >> (16 * grp)) & 0xffffull) ? 1.0f : 0.0f;
            const bool near = has_goal && !cem_task_is_nan(nsum) && cem_f2key(nsum) <= kr2;
            if (st > 0) {
                const int t = st - 1;
                const float *const at = act + (size_t)t * A;
                float u = 0.f, v = 0.f;
                if constexpr (TRACK) {
                    const float *const ap = t > 0 ? at - A : aprev;
                    for (int j = 0; j < A; ++j) {
                        const float a = at[j];
                        const float e = a - ap[j];
                        u = u + p.rho[j] * (a * a);
                        v = v + p.kappa[j] * (e * e);
                    }
                } else {
                    for (int j = 0; j < A; ++j) { const float a = at[j]; u = u + p.rho[j] * (a * a); }
                }
                const bool ga = near_prev;
                float r = (-phi) - u;
                if constexpr (TRACK) r = r - v;
                if constexpr (ZONED) r = r - pen;
                r = r + (ga ? 1.0f : 0.0f) * p.reward_goal;
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

// The launch of one kind's four instantiations, k[O > 64][vec]: the argument checks of the kind, the 16-byte test, one launch.
typedef void (*cem_task_kernel_t)(const TaskParams);
template <int KIND>
hipError_t cem_task_launch(const cem_task_kernel_t (&k)[2][2], const TaskParams &p, hipStream_t st)
{
    if (p.rows < 1 || p.N < 1 || p.H < 1 || p.O < 1 || p.O > CEM_U || p.A < 1 || p.A > CEM_MAX_ACT) return hipErrorInvalidValue;
    if (KIND >= CEM_TASK_KIND_TRACKING && (p.T < 1 || !p.ref || !p.clock)) return hipErrorInvalidValue;
    if (KIND >= CEM_TASK_KIND_ZONES && (!p.zones || p.n_zones < (KIND >= CEM_TASK_KIND_OUTPUTS ? 0 : 1) || p.n_zones > CEM_TASK_MAX_ZONES)) return hipErrorInvalidValue;
    if (KIND >= CEM_TASK_KIND_OUTPUTS && (!p.out_c || !p.out_tab || !p.out_ref || p.n_outputs < 1 || p.n_outputs > CEM_TASK_MAX_OUTPUTS || (p.out_T != 1 && p.out_T != p.T)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((p.rows + CEM_TASK_ROWS_PER_BLOCK - 1) / CEM_TASK_ROWS_PER_BLOCK)), block(CEM_TASK_THREADS);
    const bool vec = p.O % 4 == 0 && (reinterpret_cast<uintptr_t>(p.traj) & 15u) == 0;
    hipLaunchKernelGGL(k[p.O > 64][vec], grid, block, 0, st, p);
    return hipGetLastError();
}
#endif
