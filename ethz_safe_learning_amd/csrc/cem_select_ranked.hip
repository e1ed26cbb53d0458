// cem_select_ranked.hip — cem_select_ranked_kernel: the one-workgroup select for populations of at most 4096 candidates, restructured
// around one fact: with 1024 threads every thread keeps its (at most four) keys in registers from the staging to the compaction, and
// needs the other threads' keys twice only — for the bucket counts and for the few keys that share the k-th key's bucket.
//
// Same SelectParams in and the same bits out as cem_select_kernel<true, false> (cem_device.h): scores_w, elite_idx in ascending
// candidate order with ties to the lower index, mu / sigma, ctrl->best / best_score / iters / done, the result block.  Five barriers
// in front of the moments (that kernel: about twelve):
//   1  staging.  All loads are issued before anything waits (ctrl->done, the old mu / sigma, the P returns of the thread's candidates);
//      every wave leaves its key min / max, the bucket counts are cleared.  Behind the barrier every wave reduces the sixteen pairs for
//      itself.  The early return on `done` is taken HERE — behind the loads, in front of the first store to memory.
//   2  the 2048 bucket counts of [kmin, kmax] and the 64 counts of 32 consecutive buckets each, by LDS atomics from registers.  Behind it
//      every wave scans for itself — the 64 group counts, a count per lane, then the 32 counts of the group that holds the k-th key —
//      and finds the k-th key's bucket and how many of its keys are taken (need1): no broadcast through LDS, none of cem_ms_find's
//      three barriers.  A thread settles its keys at once: a higher bucket is taken, a lower one is not.
//   3  the keys of the k-th key's bucket, appended to a list (at most 256; the usual CemMpc iteration has a handful).  Behind it a thread
//      ranks each key it has in that bucket against the list by (key descending, index ascending) and takes it if fewer than need1
//      come before it.  No thread learns the k-th key from another.
//   4  take flags -> wave ballots and sixteen wave totals per slice of 1024 candidates; offsets in ascending candidate order.
//   5  the elite list in LDS (and memory), for the moments' gathers.
// Adversarial populations (tests/select_cases.py) keep cem_select_kernel's level loop: a bucket with more than 256 keys is split again,
// 11 bits finer (two more barriers per level, at most three levels), and a bucket ONE key wide — everything left ties — is settled by
// index order with one block-wide count in place of the list (barrier 3).  Where every key of the bucket is taken (need1 == m) neither
// is needed.
//
// The best of the elite set needs no walk: the elites are the k largest with ties to the lower index, so their maximum is the
// population's maximum, kmax, and its lowest index is an elite.  Threads that hold kmax meet in one LDS atomic minimum.  (With NaN AMONG
// the elites — fewer than k scores that are numbers — cem_select_kernel's walk depends on how it deals candidates to threads; this
// kernel names the largest key, a number wherever there is one.)
//
// The staged key list of SelectParams' LDS layout (CEM_SEL_KIDX) is not written: nothing here reads a key from LDS but the list of
// barrier 3.  The host passes the same dynamic LDS size for both forms.
//
// The moments, the blend, the early-stop test, the best-so-far update and the result block are cem_select_kernel's, operation for
// operation and in the same order, as this unit's OWN COPY: stating them once for both kernels would have to leave the three
// instantiations of cem_select_kernel with their instruction streams, which has not been shown.  A change there belongs here too
// (tests/test_gpu_select_ranked.py compares the two forms bit for bit).
#define CEM_DEVICE_PRIMITIVES_ONLY
#include "cem_select_ranked.h"

#define CEM_SR_LIST_MAX 256u             // keys of the k-th key's bucket that are ranked against each other (cem_select_kernel's bound)

// Wave-wide scans and reductions on the DPP path — row shifts by 1, 2, 4, 8 inside the rows of 16 lanes, then gfx9's two row broadcasts
// (lane 15 of a row into the next row, lane 31 into the upper half): six vector instructions, where six shuffles are six LDS-crossbar
// round trips.  Every wave of this kernel scans for itself, sixteen waves on four SIMDs, so what a scan issues is paid four times over.
// All 64 lanes are active wherever these are called.  A lane without a source takes `ID`, the operation's identity.
#define CEM_SR_DPP(ID, V, CTRL, ROWS) ((uint32_t)__builtin_amdgcn_update_dpp((int)(ID), (int)(V), (CTRL), (ROWS), 0xf, false))
#define CEM_SR_WAVE_STEPS(OP, ID, V) do { \
        V = OP(V, CEM_SR_DPP(ID, V, 0x111, 0xf)); V = OP(V, CEM_SR_DPP(ID, V, 0x112, 0xf)); \
        V = OP(V, CEM_SR_DPP(ID, V, 0x114, 0xf)); V = OP(V, CEM_SR_DPP(ID, V, 0x118, 0xf)); \
        V = OP(V, CEM_SR_DPP(ID, V, 0x142, 0xa)); V = OP(V, CEM_SR_DPP(ID, V, 0x143, 0xc)); } while (0)
__device__ __forceinline__ uint32_t cem_sr_add(const uint32_t a, const uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t cem_sr_min(const uint32_t a, const uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t cem_sr_max(const uint32_t a, const uint32_t b) { return a > b ? a : b; }
// inclusive prefix sum over lanes 0 .. lane
__device__ __forceinline__ uint32_t cem_sr_wave_scan(uint32_t v) { CEM_SR_WAVE_STEPS(cem_sr_add, 0u, v); return v; }
// minimum / maximum over the wave, in every lane
__device__ __forceinline__ uint32_t cem_sr_wave_min(uint32_t v) { CEM_SR_WAVE_STEPS(cem_sr_min, 0xFFFFFFFFu, v); return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }
__device__ __forceinline__ uint32_t cem_sr_wave_max(uint32_t v) { CEM_SR_WAVE_STEPS(cem_sr_max, 0u, v); return (uint32_t)__builtin_amdgcn_readlane((int)v, 63); }

// bits of a ballot below this lane
__device__ __forceinline__ uint32_t cem_sr_below(const uint64_t b) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u)); }

// In 64 consecutive counts (one per lane), the position b whose suffix sum reaches `need`: gt(b) < need <= gt(b) + count[b], gt(b) = the
// counts above b.  -> b, need - gt(b), count[b]; in every lane.  (need <= the sum of the counts, by the caller.)
__device__ __forceinline__ void cem_sr_find(const uint32_t cnt, const uint32_t need, int &b, uint32_t &need_in, uint32_t &m)
{
    const uint32_t inc = cem_sr_wave_scan(cnt);
    const uint32_t gt = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63) - inc;
    const uint64_t who = __builtin_amdgcn_ballot_w64(gt < need && need <= gt + cnt);      // one lane
    b = who ? __builtin_ctzll(who) : 0;
    need_in = need - (uint32_t)__builtin_amdgcn_readlane((int)gt, b);
    m = (uint32_t)__builtin_amdgcn_readlane((int)cnt, b);
}

// Offsets of a thread's four slices from sixteen wave totals per slice, tot[16 j + wave]: off[j] = what slices below j hold + what lower
// waves hold of slice j — the exclusive prefix of the 64 totals at 16 j + wv, one total per lane
__device__ __forceinline__ void cem_sr_offsets(const uint32_t *tot, const int lane, const int wv, uint32_t off[4])
{
    const uint32_t v = tot[lane], ex = cem_sr_wave_scan(v) - v;
    const int w = __builtin_amdgcn_readfirstlane(wv);
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = (uint32_t)__builtin_amdgcn_readlane((int)ex, 16 * j + w);
}

__global__ __launch_bounds__(1024) void cem_select_ranked_kernel(const SelectParams p)
{
    extern __shared__ __attribute__((aligned(16))) char sel_smem[];
    __shared__ __attribute__((aligned(16))) float red[4096];   // bucket counts + the bucket's list, then the moments' partial sums
    __shared__ __attribute__((aligned(16))) uint32_t wmm[2][16];     // per wave: key min, key max
    __shared__ __attribute__((aligned(16))) uint32_t wtot[64];       // per slice and wave, [16 slice + wave]: keys taken
    __shared__ __attribute__((aligned(16))) uint32_t etot[64];       // the same: keys of a one-key bucket
    __shared__ __attribute__((aligned(16))) uint32_t coarse[64];     // keys per 32 consecutive buckets
    __shared__ uint32_t sh_cnt;
    __shared__ int sh_best;
    const int prob = (int)blockIdx.x;
    CtrlBlock *const ctrl = p.ctrl + prob;
    // requested first, looked at behind barrier 1.  (A relaxed atomic load: a vector load, in flight with the returns' loads, where a plain
    // load of this uniform address is a scalar load the wave waits for at once.)
    const int done = p.check_done ? __hip_atomic_load(&ctrl->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : 0;
    const float *const scores_b = p.scores + (size_t)prob * p.N;
    const float *const actions_b = p.actions + (size_t)prob * p.N * p.HA;
    float *const musig_b = p.musig + (size_t)prob * 2 * p.HA;
    int32_t *const elite_b = p.elite_idx + (size_t)prob * p.k;
    const float *const ret_b = p.ret ? p.ret + (size_t)prob * p.P * p.N : p.ret;
    float *const scores_wb = p.scores_w ? p.scores_w + (size_t)prob * p.N : p.scores_w;

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int N = p.N, k = p.k, HA = p.HA;
    CEM_SEL_STAMP(0);
    int32_t *elite = reinterpret_cast<int32_t *>(sel_smem);                 // [k]
    float *colmean = reinterpret_cast<float *>(sel_smem + (size_t)((k + 3) & ~3) * 4);   // [HA]
    float *newsig = colmean + HA;                                           // [HA] smoothed sigma
    uint32_t *h2k = reinterpret_cast<uint32_t *>(red);                      // [2048] bucket counts
    uint32_t *lkey = h2k + 2048, *lidx = lkey + 1024;                       // the k-th key's bucket: keys, candidate indices

    // old mu / sigma of the columns this thread will finish (first column block): requested now, needed at the very end
    float old_mu = 0.f, old_sg = 0.f;
    if (tid < HA) { old_mu = musig_b[tid]; old_sg = musig_b[HA + tid]; }

    // ---- staging: candidate j * 1024 + tid is this thread's key j ------------------------------------------------
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (ret_b) {
        // cem_reduce_kernel's sum for this thread's four candidates: particles in ascending order, eight (clamped, hence
        // unconditional) loads per candidate in flight; reduce_mean = sum / P
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int q0 = 0; q0 < p.P; q0 += 8) {
            float r[8][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j * 1024 < N) {                                   // (block-uniform: a slice of 1024 candidates that exists)
                    const int i = j * 1024 + tid, ic = i < N ? i : N - 1;
#pragma unroll
                    for (int u = 0; u < 8; ++u) r[u][j] = ret_b[(size_t)(q0 + u < p.P ? q0 + u : p.P - 1) * N + ic];
                }
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (q0 + u < p.P) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) if (j * 1024 < N) acc[j] = acc[j] + r[u][j];
                }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = acc[j] / (float)p.P;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) { const int i = j * 1024 + tid; if (i < N) v[j] = scores_b[i]; }
    }
    uint32_t key[4];
    uint32_t play = 0u;                   // bit j: key j is still in the k-th key's bucket (to begin with: it exists)
    uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool in = j * 1024 + tid < N;
        key[j] = in ? cem_f2key(v[j]) : 0u;
        if (in) { play |= 1u << j; kmin = key[j] < kmin ? key[j] : kmin; kmax = key[j] > kmax ? key[j] : kmax; }
    }
    kmin = cem_sr_wave_min(kmin); kmax = cem_sr_wave_max(kmax);
    if (lane == 0) { wmm[0][wv] = kmin; wmm[1][wv] = kmax; }
    h2k[tid] = 0u; h2k[tid + 1024] = 0u;
    if (tid < 64) coarse[tid] = 0u;
    if (tid == 0) { sh_cnt = 0u; sh_best = 0x7fffffff; }
    for (int e = tid; e < k; e += 1024) elite[e] = 0;         // (exactly k entries are written below; no gather reads a word that was not)
    __syncthreads();                                                        // ---- barrier 1
    if (__builtin_amdgcn_readfirstlane(done)) return;         // (workgroup-uniform; nothing has been stored to memory)
    kmin = cem_sr_wave_min(wmm[0][lane & 15]); kmax = cem_sr_wave_max(wmm[1][lane & 15]);      // (every wave, the sixteen pairs)
    if (scores_wb) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if ((play >> j) & 1u) scores_wb[j * 1024 + tid] = v[j];
    }
    // the best of elite: the population's largest key at its lowest index (a thread's keys are in ascending candidate order)
    {
        int mine = 0x7fffffff;
#pragma unroll
        for (int j = 3; j >= 0; --j) if (((play >> j) & 1u) && key[j] == kmax) mine = j * 1024 + tid;
        if (mine != 0x7fffffff) atomicMin(&sh_best, mine);
    }
    CEM_SEL_STAMP(1);

    // ---- the k-th largest key's bucket; every key outside it is settled on the way ---------------------------------
    // 2048 buckets of the range the keys in play span, bucket = (key - base) >> sh, monotone in the key (cem_select_kernel, round 4)
    uint32_t base = kmin, need = (uint32_t)k;
    int sh; { const uint32_t window = kmax - kmin; sh = window ? max(0, 21 - (int)__clz((int)window)) : 0; }   // window >> sh < 2048
    uint32_t take = 0u;                   // bit j: key j is an elite
    uint32_t need1 = 0u, m = 0u;          // of the m keys in the k-th key's bucket the first need1 by (key descending, index ascending) are taken
#pragma unroll 1
    for (int level = 0; level < 4; ++level) {
        if (level) {                      // (every wave is done with the last level's counts before they are cleared)
            __syncthreads();
            h2k[tid] = 0u; h2k[tid + 1024] = 0u;
            if (tid < 64) coarse[tid] = 0u;
            __syncthreads();
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((play >> j) & 1u) { const uint32_t b = (key[j] - base) >> sh; atomicAdd(&h2k[b], 1u); atomicAdd(&coarse[b >> 5], 1u); }
        __syncthreads();                                                    // ---- barrier 2
        // ge[b] = #keys in buckets >= b; the one bucket with ge[b] >= need > ge[b + 1].  Every wave for itself, in two steps of 64 counts:
        // the group of 32 buckets (a lane per group), then the bucket inside it (its 32 counts in the lower lanes).
        int grp, q;
        uint32_t need_in, unused;
        cem_sr_find(coarse[lane], need, grp, need_in, unused);
        cem_sr_find(lane < 32 ? h2k[grp * 32 + lane] : 0u, need_in, q, need1, m);
        const uint32_t bucket = (uint32_t)(grp * 32 + q);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((play >> j) & 1u) {
                const uint32_t b = (key[j] - base) >> sh;
                if (b > bucket) take |= 1u << j;
                if (b != bucket) play &= ~(1u << j);
            }
        if (sh == 0 || m <= CEM_SR_LIST_MAX || need1 >= m) break;           // (workgroup-uniform)
        base += bucket << sh; need = need1;                                 // split that bucket, 11 bits finer
        sh = sh > 11 ? sh - 11 : 0;
    }
    if (need1 >= m) take |= play;                                           // the whole bucket is elite
    else if (sh == 0) {
        // the bucket is ONE key: its keys tie, the need1 of lowest candidate index are taken
        uint64_t eb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            eb[j] = __builtin_amdgcn_ballot_w64(((play >> j) & 1u) != 0u);
            if (lane == 0) etot[16 * j + wv] = (uint32_t)__builtin_popcountll(eb[j]);
        }
        __syncthreads();                                                    // ---- barrier 3 (ties)
        uint32_t off[4];
        cem_sr_offsets(etot, lane, wv, off);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (((play >> j) & 1u) && off[j] + cem_sr_below(eb[j]) < need1) take |= 1u << j;
    } else {
        // a handful of keys — the usual CemMpc case: whoever holds one ranks it against the list
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((play >> j) & 1u) {
                const uint32_t pos = atomicAdd(&sh_cnt, 1u);
                if (pos < 1024u) { lkey[pos] = key[j]; lidx[pos] = (uint32_t)(j * 1024 + tid); }
            }
        __syncthreads();                                                    // ---- barrier 3 (list)
        if (play) {
            uint32_t before[4] = {0u, 0u, 0u, 0u};
            for (uint32_t l = 0; l < m; ++l) {
                const uint32_t kl = lkey[l], il = lidx[l];
#pragma unroll
                for (int j = 0; j < 4; ++j) before[j] += (kl > key[j]) || (kl == key[j] && il < (uint32_t)(j * 1024 + tid));
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) if (((play >> j) & 1u) && before[j] < need1) take |= 1u << j;
        }
    }
    CEM_SEL_STAMP(2);

    // ---- compaction in ascending candidate index (slice by slice, wave by wave, lane by lane) -----------------------
    {
        uint64_t tb[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            tb[j] = __builtin_amdgcn_ballot_w64(((take >> j) & 1u) != 0u);
            if (lane == 0) wtot[16 * j + wv] = (uint32_t)__builtin_popcountll(tb[j]);
        }
        __syncthreads();                                                    // ---- barrier 4
        uint32_t off[4];
        cem_sr_offsets(wtot, lane, wv, off);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((take >> j) & 1u) {
                const uint32_t pos = off[j] + cem_sr_below(tb[j]);
                if (pos < (uint32_t)k) { elite[pos] = j * 1024 + tid; elite_b[pos] = j * 1024 + tid; }     // (exactly k are taken; held to the list all the same)
            }
    }
    __syncthreads();                                                        // ---- barrier 5

    CEM_SEL_STAMP(3);

    CEM_SEL_STAMP(4);
    // ---- moments over the elite set (tf.nn.moments: mean, then mean squared difference): cem_select_kernel's, copied -----------
    const float fk = (float)k;
    const float sm = p.smoothing, osm = p.one_minus_smoothing;
    // Wide path for large elite sets: a thread gathers whole float4s of an elite's action row.  Partial sums add up in a fixed order
    // (elite index ascending within a part, parts ascending).
    int tpc1 = 1; { const int nc = HA < 1024 ? HA : 1024; while (tpc1 * 2 * nc <= 1024) tpc1 *= 2; }
    if ((HA & 3) == 0 && HA <= 4096 && k > 16 * tpc1) {
        const int ncol4 = HA >> 2;
        int tpc = 1; while (tpc * 2 * ncol4 <= 1024) tpc *= 2;
        const int part = tid / ncol4, c4 = tid % ncol4;
        const bool act = part < tpc;
        f4 *red4 = reinterpret_cast<f4 *>(red);
        const f4 *act4 = reinterpret_cast<const f4 *>(actions_b);
        const f4 zero4 = (f4){0.f, 0.f, 0.f, 0.f};
        f4 av[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = part + j * tpc;
            av[j] = (act && e < k) ? act4[(size_t)elite[e] * ncol4 + c4] : zero4;
        }
        f4 mean4 = zero4;
        for (int phase = 0; phase < 2; ++phase) {
            f4 acc = zero4;
            if (act) {
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (part + j * tpc < k) { const f4 a = av[j]; acc = phase ? acc + (a - mean4) * (a - mean4) : acc + a; }
                for (int e0 = part + 8 * tpc; e0 < k; e0 += 8 * tpc) {
                    f4 b[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) { const int e = e0 + j * tpc; b[j] = e < k ? act4[(size_t)elite[e] * ncol4 + c4] : zero4; }
#pragma unroll
                    for (int j = 0; j < 8; ++j)
                        if (e0 + j * tpc < k) { const f4 a = b[j]; acc = phase ? acc + (a - mean4) * (a - mean4) : acc + a; }
                }
            }
            __syncthreads();
            red4[tid] = acc;
            __syncthreads();
            if (part == 0) {
                f4 tot = zero4;
                for (int pp = 0; pp < tpc; ++pp) tot = tot + red4[pp * ncol4 + c4];
                if (!phase) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) colmean[4 * c4 + r] = tot[r] / fk;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float sd = sqrtf(tot[r] / fk);
                        const int ci = 4 * c4 + r;
                        const float nsg = sm * musig_b[HA + ci] + osm * sd;                // cem_mpc.py:65
                        musig_b[ci] = sm * musig_b[ci] + osm * colmean[ci];                // cem_mpc.py:64
                        musig_b[HA + ci] = nsg;
                        newsig[ci] = nsg;
                    }
                }
            }
            __syncthreads();
            if (!phase && act) {
#pragma unroll
                for (int r = 0; r < 4; ++r) mean4[r] = colmean[4 * c4 + r];
            }
        }
    } else {
        for (int cb = 0; cb < HA; cb += 1024) {
            const int ncol = (HA - cb < 1024) ? HA - cb : 1024;
            int tpc = 1; while (tpc * 2 * ncol <= 1024) tpc *= 2;
            const int part = tid / ncol, col = tid % ncol;
            const bool act = part < tpc;
            // this thread's elite rows e = part, part + tpc, ...: the first 16 are gathered at once and kept for both phases
            float av[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int e = part + j * tpc;
                av[j] = (act && e < k) ? actions_b[(size_t)elite[e] * HA + cb + col] : 0.f;
            }
            for (int phase = 0; phase < 2; ++phase) {
                float acc = 0.f;
                const float mc = phase ? colmean[cb + col] : 0.f;
                if (act) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int e = part + j * tpc;
                        if (e < k) { const float a = av[j]; acc = phase ? acc + (a - mc) * (a - mc) : acc + a; }
                    }
                    for (int e0 = part + 16 * tpc; e0 < k; e0 += 8 * tpc) {      // large k: 8 gathers in flight, same summation order
                        float b[8];
#pragma unroll
                        for (int j = 0; j < 8; ++j) { const int e = e0 + j * tpc; b[j] = e < k ? actions_b[(size_t)elite[e] * HA + cb + col] : 0.f; }
#pragma unroll
                        for (int j = 0; j < 8; ++j)
                            if (e0 + j * tpc < k) { const float a = b[j]; acc = phase ? acc + (a - mc) * (a - mc) : acc + a; }
                    }
                }
                __syncthreads();
                red[tid] = acc;
                __syncthreads();
                if (part == 0) {
                    float tot = 0.f;
                    for (int pp = 0; pp < tpc; ++pp) tot = tot + red[pp * ncol + col];
                    if (!phase) colmean[cb + col] = tot / fk;
                    else {
                        const float sd = sqrtf(tot / fk);
                        const int ci = cb + col;
                        const float omu = cb == 0 ? old_mu : musig_b[ci], osg = cb == 0 ? old_sg : musig_b[HA + ci];
                        const float nsg = sm * osg + osm * sd;                             // cem_mpc.py:65
                        musig_b[ci] = sm * omu + osm * colmean[ci];                        // cem_mpc.py:64
                        musig_b[HA + ci] = nsg;
                        newsig[ci] = nsg;
                    }
                }
                __syncthreads();
            }
        }
    }
    CEM_SEL_STAMP(5);
    uint32_t *res_l = reinterpret_cast<uint32_t *>(red);     // [36] the plan's result in the making + [36] "this select completes the plan"  (LDS: the moments are done with `red`)
    if (p.result && tid < 37) res_l[tid] = 0u;
    if (p.result) __syncthreads();
    if (tid == 0) {
        float ssum = 0.f;
        for (int i = 0; i < HA; ++i) ssum = ssum + newsig[i];
        const float mean_sigma = ssum / (float)HA;
        const int iters = ctrl->iters + 1;
        const bool stop = mean_sigma <= p.threshold;                                          // cem_mpc.py:66-67
        ctrl->iters = iters;
        if (stop) ctrl->done = 1;
        if (p.result) {             // (the select that ends the plan — its last iteration or the early stop — hands the result to the host)
            res_l[33] = (uint32_t)iters; res_l[34] = stop ? 1u : (uint32_t)ctrl->done; res_l[35] = (uint32_t)ctrl->fault;
            res_l[36] = (stop || p.is_last != 0) ? 1u : 0u;
        }
        CEM_SEL_STAMP(6);
    }
    if (tid == 64) {
        const float bs = cem_key2f(kmax);                                    // the best of elite: score and candidate index
        const int idx = (uint32_t)sh_best < (uint32_t)N ? sh_best : 0;       // (some thread holds kmax; held to the population all the same)
        const bool better = bs > ctrl->best_score;                         // strict (cem_mpc.py:58)
        for (int a0 = 0; a0 < p.A; a0 += 4) {
            f4 e = (f4){0.f, 0.f, 0.f, 0.f};                                                    // the output noise of these four actions: one draw
            if (p.result && !p.eps_out) e = cem_normal4((uint32_t)(a0 >> 2), 0u, 0u, 0u, CEM_STREAM_OUT, cem_key(ctrl));
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = a0 + r;
                if (a < p.A) {
                    const float b = better ? actions_b[(size_t)idx * HA + a] : ctrl->best[a];     // first step's action
                    if (better) ctrl->best[a] = b;
                    if (p.result) res_l[a] = __float_as_uint(b + (p.eps_out ? p.eps_out[a] : e[r]) * p.noise_stddev);   // cem_mpc.py:68
                }
            }
        }
        if (better) ctrl->best_score = bs;
        if (p.result) res_l[32] = __float_as_uint(better ? bs : ctrl->best_score);
    }
    if (p.result) {
        __syncthreads();
        if (tid < 64 && res_l[36]) cem_emit_result(p.result, p.result_dev, res_l, ctrl->seq, tid);
    }
}

hipError_t prepare_select_ranked(size_t bytes)
{
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_select_ranked_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

hipError_t launch_select_ranked(const SelectParams &p, int n_problems, size_t lds_bytes, hipStream_t st)
{
    hipLaunchKernelGGL(cem_select_ranked_kernel, dim3(n_problems), dim3(1024), lds_bytes, st, p);
    return hipGetLastError();
}
