// cem_pack.h — the weight images of the rollout kernels, packed ON THE DEVICE from a natural (Keras-layout) blob that already lives
// there (cem_planner_set_weights_dev: the trainer's workspace after a fit).  Bit for bit what the host packers of cem_capi.hip
// (pack_member, pack_member_chunked, pack_member_wide + the bias rows of cem_planner_set_weights) upload.
//
// Destination driven: every image is a sequence of UNITS of 64 lanes; a lane owns the 16 bytes (fp32, wide) or the 3 x 16 bytes (split:
// one per bf16 plane) of its unit and gathers what belongs there, so every word of a member's image is written — zero padding past
// in_dim / out_dim, all-zero layer-0 blocks and the slack behind the last group included — and a wave's stores are 1 KB contiguous.
// Which matrix block a unit holds is a pure function of the shape: the host writes it down ONCE per handle as a table of PackDesc, in
// the loops of its own packers (cem_perm_l0 / cem_perm_hidden / cem_split_perm / cem_wide_base order; cem_capi.hip build_pack_table),
// and the kernels read one descriptor per wave.  The table is the same for every member.
//   fp32   unit = one accumulator half of a 2 KB group: [lane(64)][r(4)] fp32; lane 16 q + i, word r = W[16 kb + 4 q + r][16 ob + i]
//   wide   unit = one 1 KB group of cem_rollout_wide.h: the same map
//   split  unit = the a or b half of a 6 KB group: [plane(3)][lane(64)][s(8)] bf16; lane 16 q + i, slot s = piece `plane` of
//          W[16 (2 kb + s / 4) + 4 q + s % 4][16 ob + i]   (cem_split3_bits: the host's split, and -ffp-contract=off here as there)
//   bf16   unit = the a or b half of a 2 KB group of cem_rollout_bf16.h: [lane(64)][s(8)] bf16, the same slots, each weight rounded
//          once (cem_rn_bf16_bits).  Its kernel, cem_pack_bf16_kernel, lives in cem_rollout_bf16.hip, which takes the types and helpers
//          of this header (CEM_DEVICE_PRIMITIVES_ONLY, as with cem_device.h) and none of its kernels.
// The gathered reads run along the output index for the 16 lanes of a lane group (64 B segments); the shipped ensemble is 4.4 MB in all.
// One launch per image covers all E members; no atomics, no spin loops, nothing crosses a workgroup.
#pragma once
#include "cem_device.h"
#include "cem_rollout_split.h"

// one unit of an image: the block (kb, ob) of the [in_dim][out_dim] row-major matrix at float offset `src` of the member's natural blob
// (in_dim 0: a unit of zeros)
struct PackDesc { uint32_t src; uint16_t in_dim, out_dim, kb, ob; uint32_t pad_; };
static_assert(sizeof(PackDesc) == 16, "one 16-byte load per wave");

// What a pack launch takes: the trained ensemble where it lives and the image it becomes.  (Kernels outside the planning set carry
// `train` in their symbol, which is how tests/test_warm_capi_cpu.py tells them from the kernels whose register counts it pins; these
// do through this type.)
struct cem_pack_trained_t {
    const float *blob;           // [E][nat] natural blobs (device)
    const PackDesc *desc;        // [n_desc]
    char *dst;                   // member 0's image
    float *blob_copy;            // wide: the natural blobs the wide path keeps in front of its images ([E][nat]), else null
    unsigned long long member_bytes;   // image stride of a member
    uint32_t nat;                // floats of a member's natural blob
    uint32_t n_desc;             // described units of a member
    uint32_t n_slack;            // 1 KB units of zeros behind them (the prefetch queues' slack)
    uint32_t E;
};

#define CEM_PACK_WAVES 4         // units per workgroup

__device__ __forceinline__ float cem_pack_at(const PackDesc d, const float *nat, const int k, const int o)
{
    return (k < (int)d.in_dim && o < (int)d.out_dim) ? nat[d.src + (uint32_t)k * d.out_dim + (uint32_t)o] : 0.f;
}

// unit and member of this wave (units of a member are dealt to consecutive waves; a workgroup never straddles a member)
#define CEM_PACK_WHERE(P_, UNITS_) \
    const uint32_t wgs_ = ((UNITS_) + CEM_PACK_WAVES - 1) / CEM_PACK_WAVES; \
    const uint32_t m = blockIdx.x / wgs_, unit = (blockIdx.x % wgs_) * CEM_PACK_WAVES + (threadIdx.x >> 6); \
    const int lane = threadIdx.x & 63, q = lane >> 4, i = lane & 15; \
    const float *nat = (P_).blob + (size_t)m * (P_).nat; \
    char *img = (P_).dst + (size_t)m * (P_).member_bytes

__device__ __forceinline__ f4 cem_pack_quad(const PackDesc d, const float *nat, const int q, const int i)
{
    f4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) v[r] = cem_pack_at(d, nat, 16 * d.kb + 4 * q + r, 16 * d.ob + i);
    return v;
}

// the bf16 image from cem_rollout_bf16.hip.  Weak: a library built from cem_capi.hip alone has no bf16 rollout (cem_rollout_bf16.h).
__attribute__((weak)) void launch_pack_bf16(const cem_pack_trained_t &p, unsigned grid, hipStream_t st);

#ifndef CEM_DEVICE_PRIMITIVES_ONLY   // (a second translation unit takes the types and helpers above, not the plain kernels: cem_rollout_bf16.hip)

// the tuned rollout's stream (pack_member): 2 KB groups [g(2)][lane(64)][r(4)], two units each
__global__ __launch_bounds__(64 * CEM_PACK_WAVES) void cem_pack_fp32_kernel(const cem_pack_trained_t p)
{
    CEM_PACK_WHERE(p, p.n_desc + p.n_slack);
    if (unit >= p.n_desc + p.n_slack) return;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (unit < p.n_desc) v = cem_pack_quad(p.desc[unit], nat, q, i);
    *reinterpret_cast<f4 *>(img + (size_t)unit * 1024 + lane * 16) = v;
}

// the split rollout's stream (pack_member_chunked, three planes): 6 KB groups [ab(2)][plane(3)][lane(64)][s(8)] bf16, two 3 KB units each
__global__ __launch_bounds__(64 * CEM_PACK_WAVES) void cem_pack_split_kernel(const cem_pack_trained_t p)
{
    CEM_PACK_WHERE(p, p.n_desc + p.n_slack);
    if (unit >= p.n_desc + p.n_slack) return;
    if (unit >= p.n_desc) {                                   // slack: 1 KB units behind the last group
        *reinterpret_cast<cem_u4 *>(img + (size_t)p.n_desc * 3072 + (size_t)(unit - p.n_desc) * 1024 + lane * 16) = (cem_u4){0u, 0u, 0u, 0u};
        return;
    }
    const PackDesc d = p.desc[unit];
    cem_u4 pl[3] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        const float v = cem_pack_at(d, nat, 16 * (2 * d.kb + (s >> 2)) + 4 * q + (s & 3), 16 * d.ob + i);
        unsigned a[3]; cem_split3_bits(v, a[0], a[1], a[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) pl[j][s >> 1] |= (s & 1) ? (a[j] & 0xFFFF0000u) : (a[j] >> 16);      // bf16 slot s: little endian halves
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) *reinterpret_cast<cem_u4 *>(img + (size_t)unit * 3072 + j * 1024 + lane * 16) = pl[j];
}

// the wide rollout's images (pack_member_wide): 1 KB groups in cem_wide_base / cem_wide_groups order — and the natural blobs the wide
// path keeps in front of them, copied by the same threads
__global__ __launch_bounds__(64 * CEM_PACK_WAVES) void cem_pack_wide_kernel(const cem_pack_trained_t p)
{
    CEM_PACK_WHERE(p, p.n_desc);
    for (uint32_t k = (blockIdx.x % wgs_) * blockDim.x + threadIdx.x; k < p.nat; k += wgs_ * blockDim.x)
        p.blob_copy[(size_t)m * p.nat + k] = nat[k];
    if (unit >= p.n_desc) return;
    *reinterpret_cast<f4 *>(img + (size_t)unit * 1024 + lane * 16) = cem_pack_quad(p.desc[unit], nat, q, i);
}

// The biases: rows of 128 features, zero padded, one float4 per thread.  Tuned / split handles: bias_h [E][L][128], bias_mu / bias_var
// [E][128] and the same rows of the per-member table (CEM_ET_BMU, CEM_ET_BVAR, CEM_ET_ROWS + l).  Wide handles: the table alone, a
// hidden layer's up to 256 biases in rows CEM_ET_ROWS + 2 l, + 1 (cem_planner_set_weights writes no more either).
struct cem_pack_trained_bias_t {
    const float *blob;
    float *bias_h, *bias_mu, *bias_var, *etab;
    uint32_t nat, Din, U, L, O, E, wide;
};
__global__ __launch_bounds__(256) void cem_pack_bias_kernel(const cem_pack_trained_bias_t p)
{
    const uint32_t per_layer = p.wide ? 2u : 1u, rows = 2u + per_layer * p.L, et_rows = CEM_ET_ROWS + per_layer * p.L;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t f0 = (t & 31u) * 4u, row = (t >> 5) % rows, m = (t >> 5) / rows;
    if (m >= p.E) return;
    const float *nat = p.blob + (size_t)m * p.nat;
    // natural blob offsets of the bias vectors (cem_capi.hip nat_offsets)
    const uint32_t heads = p.Din * p.U + p.U + (p.L - 1u) * (p.U * p.U + p.U);
    uint32_t src, n, first = f0, et_row;
    float *out = nullptr;
    if (row < 2u) {                                           // b_mu, b_var
        src = heads + p.U * p.O + row * (p.O + p.U * p.O); n = p.O; et_row = CEM_ET_BMU + row;
        if (!p.wide) out = (row ? p.bias_var : p.bias_mu) + (size_t)m * CEM_U;
    } else {
        const uint32_t r = row - 2u, l = r / per_layer;
        src = l == 0 ? p.Din * p.U : p.Din * p.U + p.U + (l - 1u) * (p.U * p.U + p.U) + p.U * p.U;
        n = p.U; first = f0 + (r % per_layer) * CEM_U; et_row = CEM_ET_ROWS + r;
        if (!p.wide) out = p.bias_h + ((size_t)m * p.L + l) * CEM_U;
    }
    f4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = first + j < n ? nat[src + first + j] : 0.f;
    *reinterpret_cast<f4 *>(p.etab + ((size_t)m * et_rows + et_row) * CEM_U + f0) = v;
    if (out) *reinterpret_cast<f4 *>(out + f0) = v;
}

#endif  // CEM_DEVICE_PRIMITIVES_ONLY
