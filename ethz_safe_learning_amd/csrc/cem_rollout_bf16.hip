// cem_rollout_bf16.hip — the translation unit of the precision = CEM_PRECISION_BF16 rollout (cem_rollout_bf16_kernel: cem_rollout_bf16.h
// holds it and says why it is compiled apart) and of cem_pack_bf16_kernel, the device packer of its weight image (below; the unit
// table, parameter block and helpers are cem_pack.h's).
#define CEM_DEVICE_PRIMITIVES_ONLY
#define CEM_ROLLOUT_BF16_UNIT
#include "cem_rollout_bf16.h"
#include "cem_pack.h"

// the bf16 rollout's stream (pack_member_chunked, one plane): 2 KB groups [ab(2)][lane(64)][s(8)] bf16, two 1 KB units each
__global__ __launch_bounds__(64 * CEM_PACK_WAVES) void cem_pack_bf16_kernel(const cem_pack_trained_t p)
{
    CEM_PACK_WHERE(p, p.n_desc + p.n_slack);
    if (unit >= p.n_desc + p.n_slack) return;
    cem_u4 v = {0u, 0u, 0u, 0u};
    if (unit < p.n_desc) {
        const PackDesc d = p.desc[unit];
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const unsigned a = cem_rn_bf16_bits(cem_pack_at(d, nat, 16 * (2 * d.kb + (s >> 2)) + 4 * q + (s & 3), 16 * d.ob + i));
            v[s >> 1] |= (s & 1) ? a : (a >> 16);             // bf16 slot s: little endian halves
        }
    }
    *reinterpret_cast<cem_u4 *>(img + (size_t)unit * 1024 + lane * 16) = v;
}

CEM_CHUNKED_LAUNCHER(launch_rollout_bf16, cem_rollout_bf16_kernel, 1)

void launch_pack_bf16(const cem_pack_trained_t &p, unsigned grid, hipStream_t st)
{
    hipLaunchKernelGGL(cem_pack_bf16_kernel, dim3(grid), dim3(64 * CEM_PACK_WAVES), 0, st, p);
}
