// cem_noise_mix.h — time-correlated action noise (cem_planner_set_action_noise, CEM_NOISE_MIXED): one kernel that writes
//   eps[b][i][n][t][a] = sum over u of M[t][u] * xi[b][i][n][u][a]
// once per plan, xi being the white action stream the samplers draw (cem_normal4 at (n, u, i, a / 4, CEM_STREAM_ACT), key of problem b).
// The samplers then read eps through RolloutParams::eps_act, the path every caller-supplied tensor takes (cem_sample_store), so nothing
// behind this kernel changes.
//
// The contract, per (b, i, n, a) and output step t (include/cem_mpc.h):
//   acc = +0.f;  for u = 0 .. H - 1 in order:  acc = fl32(acc + fl32(M[t][u] * xi[u]))
// multiply and add rounded separately (-ffp-contract=off), every term taken (zeros of M included), no atomics: a pure function of the
// key and M.  planner.mix_noise is the NumPy restatement; tests/test_gpu_colored_noise.py holds the two equal bit for bit.
//
// Work split: a SEQUENCE is one (iteration, candidate, action quad) — H white f4 draws in, H f4 sums out.  A 256-thread workgroup takes
// 256 / H sequences at a time (H <= 128: at least two).  Thread (sequence s, step u) draws xi[s][u] into LDS — one Philox call, exactly
// the one the sampler would have made —; behind a barrier thread (s, t) forms its four dot products over u.  M is staged once per
// workgroup in LDS, TRANSPOSED ([u][t], which is how the host uploads it): in step u of the loop the lanes of a sequence read H
// consecutive words and the lanes of another sequence in the same wave read the same words (a broadcast), so the M reads are free of
// bank conflicts whatever H is.  The xi reads are one ds_read_b128 address per sequence, broadcast to the sequence's lanes; the
// addresses of a wave's sequences lie H * 16 bytes apart, which for H = 8, 16, 32 puts them on few banks — not padded and not measured:
// the kernel runs once per plan (profiles/colored_noise.json has its time).  Workgroups stride over the groups of sequences, so M is
// staged once per workgroup, not once per group.
//
// This header is what cem_capi.hip includes; the kernel itself is compiled in a translation unit of its own (cem_noise_mix.hip defines
// CEM_NOISE_MIX_UNIT), as the lean rollout is, so that the device code of cem_capi.hip stays what it was instruction for instruction.
#pragma once
#include "cem_device.h"

#define CEM_MIX_MAX_H 128
#define CEM_MIX_THREADS 256
// dynamic LDS: xi [256 / H sequences][H] quads, then M transposed [H][H] floats (H = 128: 4 KB + 64 KB)
#define CEM_MIX_SEQS(H_) (CEM_MIX_THREADS / (H_))
#define CEM_MIX_LDS_BYTES(H_) ((size_t)CEM_MIX_SEQS(H_) * (H_) * 16 + (size_t)(H_) * (H_) * 4)

struct MixParams {
    const float *mix_t;          // [H][H] the mixing matrix transposed: mix_t[u * H + t] = M[t][u]
    float *eps;                  // [problems][I][N][H][A]
    const CtrlBlock *ctrl;       // [problems]: the Philox key, and `done` (a stopped problem of a batch handle is skipped)
    int32_t I, N, H, A;
};

// grid (min(groups of sequences, a few per CU), problems).  Weak: a library built from cem_capi.hip alone has no mixed noise and
// cem_planner_set_action_noise says so (CEM_ERR_UNSUPPORTED).
__attribute__((weak)) hipError_t launch_mix_action_noise(const MixParams &p, int n_problems, hipStream_t st);
// Outside any capture, by every handle's first MIXED setter call: the runtime grants 64 KB of dynamic LDS per workgroup by default and
// has to be asked for more.  Like the library's other kernels (the select at create, the refit in ensure_refit) this one asks from
// 48 KB up — H >= 107; below the default the request changes nothing — and for the whole H = 128 allowance at once.  The attribute is
// set on the device current at the call, which is the handle's (a handle's calls come with its device current); a handle on another
// device asks there in its own first call.
__attribute__((weak)) hipError_t prepare_mix_action_noise(int H);

#ifdef CEM_NOISE_MIX_UNIT
__global__ __launch_bounds__(CEM_MIX_THREADS) void cem_mix_action_noise_kernel(const MixParams p)
{
    extern __shared__ __attribute__((aligned(16))) char mix_smem[];
    const int b = (int)blockIdx.y;
    if (p.ctrl[b].done) return;                              // workgroup-uniform: no barrier has been reached yet
    const int H = p.H, A = p.A, AZ = (A + 3) >> 2, spb = CEM_MIX_SEQS(H);
    f4 *xi = reinterpret_cast<f4 *>(mix_smem);              // [spb][H]
    float *mt = reinterpret_cast<float *>(mix_smem + (size_t)spb * H * 16);     // [H][H], u major
    for (int e = (int)threadIdx.x; e < H * H; e += CEM_MIX_THREADS) mt[e] = p.mix_t[e];
    const PhiloxKey key = cem_key(p.ctrl + b);
    const int n_seq = p.I * p.N * AZ, n_groups = (n_seq + spb - 1) / spb;
    const int s = (int)threadIdx.x / H, t = (int)threadIdx.x - s * H;           // (threads beyond spb * H: s == spb, idle)
    float *out = p.eps + (size_t)b * p.I * p.N * H * A;
    for (int g = (int)blockIdx.x; g < n_groups; g += (int)gridDim.x) {          // (the trip count is the workgroup's: barriers inside)
        const int q = g * spb + s;                           // sequence: action quad fastest, then candidate, then iteration
        const bool live = s < spb && q < n_seq;
        const int z = q % AZ, n = (q / AZ) % p.N, it = q / (AZ * p.N);
        if (live) xi[s * H + t] = cem_normal4((uint32_t)n, (uint32_t)t, (uint32_t)it, (uint32_t)z, CEM_STREAM_ACT, key);
        __syncthreads();                                     // (the first pass: M is staged, too)
        if (live) {
            f4 acc = {0.f, 0.f, 0.f, 0.f};
            for (int u = 0; u < H; ++u) {
                const float m = mt[u * H + t];
                const f4 x = xi[s * H + u];
#pragma unroll
                for (int r = 0; r < 4; ++r) { const float pr = m * x[r]; acc[r] = acc[r] + pr; }
            }
            float *o = out + (((size_t)it * p.N + n) * H + t) * A + 4 * z;
#pragma unroll
            for (int r = 0; r < 4; ++r) if (4 * z + r < A) o[r] = acc[r];
        }
        __syncthreads();                                     // xi is drawn anew in the next pass
    }
}

hipError_t launch_mix_action_noise(const MixParams &p, int n_problems, hipStream_t st)
{
    const size_t lds = CEM_MIX_LDS_BYTES(p.H);
    const int spb = CEM_MIX_SEQS(p.H), n_seq = p.I * p.N * ((p.A + 3) / 4);
    const int n_groups = (n_seq + spb - 1) / spb;
    hipLaunchKernelGGL(cem_mix_action_noise_kernel, dim3(n_groups < 1024 ? n_groups : 1024, n_problems), dim3(CEM_MIX_THREADS), lds, st, p);
    return hipGetLastError();
}

hipError_t prepare_mix_action_noise(int H)
{
    if (CEM_MIX_LDS_BYTES(H) <= 48 * 1024) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_mix_action_noise_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CEM_MIX_LDS_BYTES(CEM_MIX_MAX_H));
}
#endif
