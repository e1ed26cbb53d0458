// cem_capi.hip — host side of the C ABI declared in include/cem_mpc.h.
// Built with: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC (see csrc/build.sh).
#include "cem_device.h"
#include "cem_rollout_lean.h"
#include "cem_score.h"
#include "cem_refit_weighted.h"
#include "cem_noise_mix.h"
#include "cem_elite_carry.h"
#include "cem_plan_readout.h"
#include "cem_select_ranked.h"
#include "cem_task_score.h"
#include "cem_task_reference.h"
#include "cem_task_zones.h"
#include "cem_task_outputs.h"
#include "cem_population.h"
#include "cem_train.h"
#include "cem_train_tile.h"
#include "cem_forward.h"
#include "cem_rollout_split.h"
#include "cem_rollout_bf16.h"
#include "cem_rollout_wide.h"
#include "cem_pack.h"
#include "../../include/cem_mpc.h"
#include "cem_plan_options.h"

#include <dlfcn.h>
#include <link.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

static thread_local int g_last_hip = 0;
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { g_last_hip = (int)e_; return CEM_ERR_HIP; } } while (0)

namespace {

struct Dims {
    int O, A, Din, U, L, E, P, N, H, k, I, W, R;
    int Nloc, n_off, Bloc, Btot;
    int KB_in, KB_obs, NFW, KF0;     // KF0 = 4*NFW: layer-0 groups per wave, zero padded so every stage is a multiple of 4
    int act_q0, act_nq;              // feature quads of the network input that hold action features: [act_q0, act_q0 + act_nq)
    bool wide;                       // units > 128 or an activation other than relu: the generic rollout kernel (cem_rollout_wide.h)
    int planes;                      // bf16 planes of the chunked rollouts (cem_rollout_chunked.h), 0 for fp32 / wide: 3 = precision CEM_PRECISION_SPLIT_BF16X3
                                     // (cem_rollout_split.h, weight stream in 6 KB chunk groups), 1 = CEM_PRECISION_BF16 (cem_rollout_bf16.h, 2 KB chunk groups)
    int G0, GS;                      // groups of a wave's stream per stage: layer 0 / every other stage (K = 32 chunks when chunked, else 16-feature blocks)
    int wave_groups[4]; uint32_t wave_off_f4[4]; uint32_t member_stride_f4;
    size_t nat_member_floats;
    bool chunked() const { return planes != 0; }
    bool split() const { return planes == 3; }      // (the two for sites that concern ONE kernel)
    bool bf16() const { return planes == 1; }
    uint32_t group_bytes() const { return chunked() ? planes * 2048u : 2048u; }
};

// Which select kernel an iteration gets (cem_mpc.h select_mode; used by validate() and enqueue_select() alike, so that what one accepts
// the other can run).  requested 0 = automatic: the one-workgroup kernel while the population is below 24 000 candidates AND that kernel
// can hold its elite list + two per-(step, action) arrays + the staged keys in dynamic LDS; otherwise the multi-workgroup forms, which
// have no such limit — fused into one launch (3) when all its workgroups can be resident at once, else the eight-launch chain (2).
// Returns 0 if the REQUESTED form cannot serve this shape (only an explicit request for the one-workgroup kernel can fail).
int resolve_select_mode(int requested, long long N, long long k, long long HA, size_t dyn_limit, bool can_fuse, bool *cache_out)
{
    const size_t base = (size_t)((k + 3) & ~3ll) * 4 + (size_t)2 * HA * 4;
    const bool one_wg_ok = k <= 24576 && base <= dyn_limit;
    const bool cache = one_wg_ok && base + (size_t)CEM_SEL_KWORDS(N) * 4 <= dyn_limit;
    if (cache_out) *cache_out = cache;
    int mode = requested;
    if (mode == 0) mode = (N >= 24000 || !cache) ? 3 : 1;
    if (mode == 1 && !one_wg_ok) return 0;
    if (mode == 3 && !can_fuse) mode = 2;
    return mode;
}

int validate(const cem_config_t *c)
{
    if (!c) return CEM_ERR_INVALID_ARG;
    if (c->abi_version != CEM_ABI_VERSION) return CEM_ERR_INVALID_ARG;
    if (c->obs_dim < 1 || c->act_dim < 1 || c->act_dim > CEM_MAX_ACT || c->n_layers < 1 || c->ensemble_size < 1 ||
        c->particles < 1 || c->n_samples < 1 || c->horizon < 1 || c->horizon > 65535 || c->iterations < 1 || c->iterations > 65535 ||
        c->n_elite < 1 || c->n_elite > c->n_samples || c->world_size < 1 || c->rank < 0 || c->rank >= c->world_size)
        return CEM_ERR_INVALID_ARG;
    if (c->units < 1) return CEM_ERR_INVALID_ARG;
    if (c->activation < CEM_ACT_RELU || c->activation > CEM_ACT_GELU) return CEM_ERR_INVALID_ARG;
    if (!(fabs((double)c->one_minus_smoothing - (1.0 - (double)c->smoothing)) <= 2e-7)) return CEM_ERR_INVALID_ARG;   // see cem_mpc.h
    if (c->units > CEM_WIDE_U) return CEM_ERR_UNSUPPORTED;  // <= 128: the fast kernel (narrower layers run zero-padded, exactly); 129..256: cem_rollout_wide.h
    if (c->obs_dim + c->act_dim > CEM_U) return CEM_ERR_UNSUPPORTED;
    if (c->n_samples % c->world_size != 0) return CEM_ERR_INVALID_ARG;
    if (((long long)c->particles * c->n_samples) % c->ensemble_size != 0) return CEM_ERR_SPLIT;
    // the ONE-workgroup select kernel keeps the elite list and two per-(step, action) arrays in dynamic LDS (140 KB available, at most
    // 24576 elites): only an explicit request for it can be refused — the automatic choice routes such shapes to the multi-workgroup forms
    if (c->select_mode >= 0 && c->select_mode <= 3 &&
        resolve_select_mode(c->select_mode, c->n_samples, c->n_elite, (long long)c->horizon * c->act_dim, 140 * 1024, true, nullptr) == 0)
        return CEM_ERR_UNSUPPORTED;
    if (c->scorer.n_cost_kinds < 0 || c->scorer.n_cost_kinds > CEM_MAX_COST_KINDS) return CEM_ERR_INVALID_ARG;
    {   // scorer slices: inside the observation and non-empty (an empty lidar slice would make closest_distance +inf and rewards NaN)
        const cem_scorer_t &s = c->scorer;
        if (s.goal_mode != 0 && s.goal_mode != 1) return CEM_ERR_INVALID_ARG;
        if (s.goal_lo < 0 || s.goal_lo >= c->obs_dim) return CEM_ERR_INVALID_ARG;
        if (s.goal_mode == 0 && (s.goal_hi <= s.goal_lo || s.goal_hi > c->obs_dim)) return CEM_ERR_INVALID_ARG;
        for (int k = 0; k < s.n_cost_kinds; ++k)
            if (s.cost_lo[k] < 0 || s.cost_hi[k] <= s.cost_lo[k] || s.cost_hi[k] > c->obs_dim) return CEM_ERR_INVALID_ARG;
        if (!(s.lidar_max_dist >= 0.f) || !(s.goal_reached_dist == s.goal_reached_dist)) return CEM_ERR_INVALID_ARG;
    }
    // flat int indices of the sample / rollout / reduce kernels: N*H*A and H*P*N/world must fit an int32
    if ((long long)c->n_samples * c->horizon * ((c->act_dim + 3) & ~3) > 0x7fffffffll) return CEM_ERR_UNSUPPORTED;
    if ((long long)c->particles * (c->n_samples / c->world_size) * c->horizon > 0x7fffffffll) return CEM_ERR_UNSUPPORTED;
    {   // the hot kernel addresses the padded action quads with 32-bit byte offsets (one buffer resource)
        const long long nq = (c->obs_dim + c->act_dim + 3) / 4 - c->obs_dim / 4;
        if ((long long)c->n_samples * c->horizon * nq * 16 > 0x7fffffffll) return CEM_ERR_UNSUPPORTED;
    }
    if (c->variant != CEM_VARIANT_CEM && c->variant != CEM_VARIANT_SAFE && c->variant != CEM_VARIANT_COST) return CEM_ERR_INVALID_ARG;
    // the cost objective's reduce is rank-local and would serve a shard as it is; no multi-rank run of it has been made, so it is not offered
    if (c->variant == CEM_VARIANT_COST && c->world_size > 1) return CEM_ERR_UNSUPPORTED;
    if (c->chunks_per_tile < 0 || c->chunks_per_tile > 4) return CEM_ERR_INVALID_ARG;
    if (c->rollout_segments < 0 || c->rollout_segments > 64) return CEM_ERR_INVALID_ARG;
    if (c->select_mode < 0 || c->select_mode > 3) return CEM_ERR_INVALID_ARG;
    if (c->precision != CEM_PRECISION_FP32 && c->precision != CEM_PRECISION_SPLIT_BF16X3 && c->precision != CEM_PRECISION_BF16) return CEM_ERR_INVALID_ARG;
    if (c->precision != CEM_PRECISION_FP32 && (c->units > CEM_U || c->activation != CEM_ACT_RELU)) return CEM_ERR_UNSUPPORTED;
    // the reduced-precision mode's arithmetic is its contract: the diagnostic that routes a handle to the generic fp32 kernel (make_dims) is refused
    if (c->precision == CEM_PRECISION_BF16 && std::getenv("CEM_FORCE_GENERIC_ROLLOUT") != nullptr) return CEM_ERR_UNSUPPORTED;
    if ((long long)c->particles * c->n_samples > (1ll << 30)) return CEM_ERR_UNSUPPORTED;
    return CEM_OK;
}

Dims make_dims(const cem_config_t *c)
{
    Dims d{};
    d.O = c->obs_dim; d.A = c->act_dim; d.Din = d.O + d.A; d.U = c->units; d.L = c->n_layers; d.E = c->ensemble_size;
    d.P = c->particles; d.N = c->n_samples; d.H = c->horizon; d.k = c->n_elite; d.I = c->iterations;
    d.W = c->world_size; d.R = c->rank;
    d.Nloc = d.N / d.W; d.n_off = d.R * d.Nloc; d.Bloc = d.P * d.Nloc; d.Btot = d.P * d.N;
    d.KB_in = (d.Din + 15) / 16; d.KB_obs = (d.O + 15) / 16; d.NFW = (d.KB_in + 3) / 4; d.KF0 = 4 * d.NFW;
    d.act_q0 = d.O / 4; d.act_nq = (d.Din + 3) / 4 - d.act_q0;
    d.wide = d.U > CEM_U || c->activation != CEM_ACT_RELU || std::getenv("CEM_FORCE_GENERIC_ROLLOUT") != nullptr;   // (the variable: a diagnostic, scripts/sweep_configs.py)
    d.planes = d.wide ? 0 : c->precision == CEM_PRECISION_SPLIT_BF16X3 ? 3 : c->precision == CEM_PRECISION_BF16 ? 1 : 0;
    // fp32 stream: 2 KB groups, one per 16-feature input block; split stream: 6 KB groups, one per K = 32 chunk (two blocks);
    // bf16 stream: 2 KB groups, one per K = 32 chunk
    d.G0 = d.chunked() ? cem_chunked_l0_chunks(d.NFW, d.split() ? CEM_SPLIT_RING : CEM_BF16_RING) : d.KF0;
    d.GS = d.chunked() ? CEM_SPLIT_CHUNKS : CEM_NG;
    uint32_t off = 0;
    for (int w = 0; w < 4; ++w) {
        int g = d.G0 + d.GS * (d.L - 1);
        for (int i = 0; i < d.NFW; ++i) if (w + 4 * i < d.KB_obs) g += d.GS;
        d.wave_groups[w] = g; d.wave_off_f4[w] = off; off += (uint32_t)g * (d.group_bytes() / 16);
    }
    d.member_stride_f4 = off + 256u;    // +2 groups of slack: the prefetch queue may run ahead of a short stream
    d.nat_member_floats = (size_t)d.Din * d.U + d.U + (size_t)(d.L - 1) * ((size_t)d.U * d.U + d.U) + 2 * ((size_t)d.U * d.O + d.O);
    return d;
}

// natural blob offsets of one member
struct NatOff { std::vector<size_t> W, b; size_t Wmu, bmu, Wvar, bvar; };
NatOff nat_offsets(const Dims &d)
{
    NatOff n; size_t o = 0; int fi = d.Din;
    for (int l = 0; l < d.L; ++l) { n.W.push_back(o); o += (size_t)fi * d.U; n.b.push_back(o); o += d.U; fi = d.U; }
    n.Wmu = o; o += (size_t)d.U * d.O; n.bmu = o; o += d.O; n.Wvar = o; o += (size_t)d.U * d.O; n.bvar = o;
    return n;
}

// Weight stream of (member, wave): A-operand order of v_mfma_f32_16x16x4_f32 for out^T = W^T h^T.
// group = [g(2)][lane(64)][r(4)]; lane = 16*kq + i holds W[k = 16F + 4kq + r][out = 16G + i]: the k-quad of
// MFMA step (F, r) is {16F + r, 16F+4 + r, 16F+8 + r, 16F+12 + r}, i.e. exactly what accumulator register r
// of the producing layer holds across the four lane groups.
void pack_member(const Dims &d, const float *nat, float *out)
{
    const NatOff no = nat_offsets(d);
    std::memset(out, 0, (size_t)d.member_stride_f4 * 4 * sizeof(float));
    for (int w = 0; w < 4; ++w) {
        float *dst = out + (size_t)d.wave_off_f4[w] * 4;
        auto emit = [&](const float *W, int in_dim, int out_dim, int ld, int F, int g, int Gout) {
            for (int lane = 0; lane < 64; ++lane) {
                const int kq = lane >> 4, i = lane & 15;
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * F + 4 * kq + r, o = 16 * Gout + i;
                    dst[((size_t)g * 64 + lane) * 4 + r] = (k < in_dim && o < out_dim) ? W[(size_t)k * ld + o] : 0.f;
                }
            }
        };
        // groups are stored in the order the wave visits them: its own input blocks first (cem_perm_l0 / cem_perm_hidden)
        for (int P = 0; P < d.KF0; ++P) {                         // layer 0 (blocks >= KB_in are all zero)
            const int F = cem_perm_l0(w, d.NFW, P);
            emit(nat + no.W[0], d.Din, d.U, d.U, F, 0, 2 * w); emit(nat + no.W[0], d.Din, d.U, d.U, F, 1, 2 * w + 1);
            dst += 512;
        }
        for (int l = 1; l < d.L; ++l)
            for (int P = 0; P < CEM_NG; ++P) {
                const int F = cem_perm_hidden(w, P), Fb = cem_perm_hidden(w, P < 2 ? (P ^ 1) : P);   // second accumulator: own blocks swapped
                emit(nat + no.W[l], d.U, d.U, d.U, F, 0, 2 * w); emit(nat + no.W[l], d.U, d.U, d.U, Fb, 1, 2 * w + 1);
                dst += 512;
            }
        for (int i = 0; i < d.NFW; ++i) {
            const int Fo = w + 4 * i;
            if (Fo >= d.KB_obs) continue;
            for (int P = 0; P < CEM_NG; ++P) {                    // heads: g=0 mu, g=1 var of obs block Fo
                const int F = cem_perm_hidden(w, P), Fb = cem_perm_hidden(w, P < 2 ? (P ^ 1) : P);
                emit(nat + no.Wmu, d.U, d.O, d.O, F, 0, Fo); emit(nat + no.Wvar, d.U, d.O, d.O, Fb, 1, Fo);
                dst += 512;
            }
        }
    }
}

// Weight stream of (member, wave) for cem_rollout_split.h: groups of 6 KB in visiting order, one per K = 32 chunk (input blocks
// 2F, 2F + 1): [a planes 0..2][b planes 0..2], a plane = [64 lanes][8 bf16].  Lane 16 q + i holds, for output feature 16 G + i, the
// chunk's k slots s = 0..7 = input features 16 (2F + s / 4) + 4 q + s % 4 — what a lane's two accumulator quads of the producing
// stage hold — as piece `plane` of the exact three-way bf16 split of the weight (cem_split3_bits).
// For cem_rollout_bf16.h (d.planes == 1): the same groups with ONE plane — 2 KB, [a][b], each [64 lanes][8 bf16], the same k slots in the
// same visiting order — every weight rounded to bf16 once, to nearest even (cem_rn_bf16_bits).
void pack_member_chunked(const Dims &d, const float *nat, uint16_t *out)
{
    const NatOff no = nat_offsets(d);
    const int planes = d.planes, group = planes * 1024;           // uint16 per group
    std::memset(out, 0, (size_t)d.member_stride_f4 * 16);
    for (int w = 0; w < 4; ++w) {
        uint16_t *dst = out + (size_t)d.wave_off_f4[w] * 8;
        auto emit = [&](const float *W, int in_dim, int out_dim, int ld, int F, int ab, int Gout) {
            for (int lane = 0; lane < 64; ++lane) {
                const int kq = lane >> 4, i = lane & 15;
                for (int s = 0; s < 8; ++s) {
                    const int k = 16 * (2 * F + (s >> 2)) + 4 * kq + (s & 3), o = 16 * Gout + i;
                    const float v = (k < in_dim && o < out_dim) ? W[(size_t)k * ld + o] : 0.f;
                    unsigned a[3] = {cem_rn_bf16_bits(v), 0u, 0u};
                    if (planes == 3) cem_split3_bits(v, a[0], a[1], a[2]);
                    for (int pl = 0; pl < planes; ++pl) dst[((size_t)(ab * planes + pl) * 64 + lane) * 8 + s] = (uint16_t)(a[pl] >> 16);
                }
            }
        };
        for (int P = 0; P < d.G0; ++P) {                          // layer 0: chunks in ascending order (no own chunk); chunks past the input are zero
            emit(nat + no.W[0], d.Din, d.U, d.U, P, 0, 2 * w); emit(nat + no.W[0], d.Din, d.U, d.U, P, 1, 2 * w + 1);
            dst += group;
        }
        for (int l = 1; l < d.L; ++l)
            for (int P = 0; P < CEM_SPLIT_CHUNKS; ++P) {
                const int F = cem_split_perm(w, P);
                emit(nat + no.W[l], d.U, d.U, d.U, F, 0, 2 * w); emit(nat + no.W[l], d.U, d.U, d.U, F, 1, 2 * w + 1);
                dst += group;
            }
        for (int i = 0; i < d.NFW; ++i) {
            const int Fo = w + 4 * i;
            if (Fo >= d.KB_obs) continue;
            for (int P = 0; P < CEM_SPLIT_CHUNKS; ++P) {          // heads: a = mean, b = variance of observation block Fo
                const int F = cem_split_perm(w, P);
                emit(nat + no.Wmu, d.U, d.O, d.O, F, 0, Fo); emit(nat + no.Wvar, d.U, d.O, d.O, F, 1, Fo);
                dst += group;
            }
        }
    }
}

// Weight image of one member for cem_rollout_wide_kernel: 1 KB groups [64 lanes][4] in cem_wide_base / cem_wide_groups order;
// lane (q, j), word r of group (k block kb, output block ob) = W[16 kb + 4 q + r][16 ob + j], zero past the matrix.
// rows of the per-member feature table (RolloutParams::etab): the wide kernel's hidden layers are up to 256 features = two rows each
size_t etab_rows(const Dims &d) { return CEM_ET_ROWS + (d.wide ? 2 : 1) * (size_t)d.L; }
size_t wide_image_floats(const Dims &d) { return (size_t)cem_wide_groups(d.L, d.KB_in, (d.U + 15) / 16, d.KB_obs) * 256; }
void pack_member_wide(const Dims &d, const float *nat, float *out)
{
    const NatOff no = nat_offsets(d);
    const int nbU = (d.U + 15) / 16, nbIn = d.KB_in, nbO = d.KB_obs;
    auto emit = [&](const float *W, int in_dim, int out_dim, int g, int kb, int ob) {
        float *dst = out + (size_t)g * 256;
        for (int lane = 0; lane < 64; ++lane) {
            const int q = lane >> 4, j = lane & 15;
            for (int r = 0; r < 4; ++r) {
                const int k = 16 * kb + 4 * q + r, o = 16 * ob + j;
                dst[lane * 4 + r] = (k < in_dim && o < out_dim) ? W[(size_t)k * out_dim + o] : 0.f;
            }
        }
    };
    for (int l = 0; l < d.L; ++l) {
        const int in = l == 0 ? d.Din : d.U, nbK = l == 0 ? nbIn : nbU, gl = cem_wide_base(l, nbIn, nbU);
        for (int kb = 0; kb < nbK; ++kb)
            for (int ob = 0; ob < nbU; ++ob) emit(nat + no.W[l], in, d.U, gl + kb * nbU + ob, kb, ob);
    }
    const int gh = cem_wide_base(d.L, nbIn, nbU);
    for (int kb = 0; kb < nbU; ++kb)
        for (int ob = 0; ob < nbO; ++ob) {
            emit(nat + no.Wmu, d.U, d.O, gh + kb * nbO + ob, kb, ob);
            emit(nat + no.Wvar, d.U, d.O, gh + nbU * nbO + kb * nbO + ob, kb, ob);
        }
}

// The unit table of cem_pack.h for this shape: which matrix block every unit of a member's image holds, written down in the loops of
// the three packers above (same order, same permutations), so that the device kernels gather what those packers store.
std::vector<PackDesc> build_pack_table(const Dims &d)
{
    const NatOff no = nat_offsets(d);
    std::vector<PackDesc> t;
    auto unit = [&](size_t src, int in_dim, int out_dim, int kb, int ob) {
        PackDesc u{}; u.src = (uint32_t)src; u.in_dim = (uint16_t)in_dim; u.out_dim = (uint16_t)out_dim; u.kb = (uint16_t)kb; u.ob = (uint16_t)ob;
        t.push_back(u);
    };
    if (d.wide) {
        const int nbU = (d.U + 15) / 16, nbIn = d.KB_in, nbO = d.KB_obs;
        for (int l = 0; l < d.L; ++l) {
            const int in = l == 0 ? d.Din : d.U, nbK = l == 0 ? nbIn : nbU;
            for (int kb = 0; kb < nbK; ++kb)
                for (int ob = 0; ob < nbU; ++ob) unit(no.W[l], in, d.U, kb, ob);         // group cem_wide_base(l) + kb * nbU + ob
        }
        for (int kb = 0; kb < nbU; ++kb) for (int ob = 0; ob < nbO; ++ob) unit(no.Wmu, d.U, d.O, kb, ob);
        for (int kb = 0; kb < nbU; ++kb) for (int ob = 0; ob < nbO; ++ob) unit(no.Wvar, d.U, d.O, kb, ob);
        return t;
    }
    for (int w = 0; w < 4; ++w) {                         // the waves' streams follow each other (Dims::wave_off_f4)
        const bool chunked = d.chunked();                 // K = 32 chunks in cem_split_perm order (else 16-feature blocks, cem_perm_*)
        const int per_stage = d.GS;
        for (int P = 0; P < d.G0; ++P) {
            const int F = chunked ? P : cem_perm_l0(w, d.NFW, P);
            unit(no.W[0], d.Din, d.U, F, 2 * w); unit(no.W[0], d.Din, d.U, F, 2 * w + 1);
        }
        for (int l = 1; l < d.L; ++l)
            for (int P = 0; P < per_stage; ++P) {
                const int F = chunked ? cem_split_perm(w, P) : cem_perm_hidden(w, P);
                const int Fb = chunked ? F : cem_perm_hidden(w, P < 2 ? (P ^ 1) : P);     // fp32: the second accumulator takes its own blocks swapped
                unit(no.W[l], d.U, d.U, F, 2 * w); unit(no.W[l], d.U, d.U, Fb, 2 * w + 1);
            }
        for (int i = 0; i < d.NFW; ++i) {
            const int Fo = w + 4 * i;
            if (Fo >= d.KB_obs) continue;
            for (int P = 0; P < per_stage; ++P) {
                const int F = chunked ? cem_split_perm(w, P) : cem_perm_hidden(w, P);
                const int Fb = chunked ? F : cem_perm_hidden(w, P < 2 ? (P ^ 1) : P);
                unit(no.Wmu, d.U, d.O, F, Fo); unit(no.Wvar, d.U, d.O, Fb, Fo);
            }
        }
    }
    return t;
}

struct Tile6 { int32_t v[6]; };

// tiles of one particle-major row space.  Rows r = p*nstride + n (n in [n_lo, n_hi)) use member
// (p*N + n) / chunk; a tile never straddles a member boundary (mlp_ensemble.py:123-126).
void build_plan_tiles(const Dims &d, int rc, std::vector<Tile6> &out)
{
    out.clear();
    const long long chunk = (long long)d.Btot / d.E;
    const int rows_per_tile = 16 * rc;
    for (int p = 0; p < d.P; ++p) {
        int n = d.n_off; const int n_end = d.n_off + d.Nloc;
        while (n < n_end) {
            const long long rg = (long long)p * d.N + n;
            const int member = (int)(rg / chunk);
            const long long seg_end_g = std::min<long long>((long long)(member + 1) * chunk, (long long)p * d.N + n_end);
            const int seg = (int)(seg_end_g - rg);
            const int ntile = (seg + rows_per_tile - 1) / rows_per_tile;
            int done = 0;
            for (int t = 0; t < ntile; ++t) {
                const int cnt = (seg - done + (ntile - t) - 1) / (ntile - t);     // even split
                Tile6 td; td.v[0] = p * d.Nloc + (n - d.n_off) + done; td.v[1] = cnt; td.v[2] = member;
                td.v[3] = n + done; td.v[4] = (int)(rg + done); td.v[5] = -1;
                out.push_back(td); done += cnt;
            }
            n += seg;
        }
    }
    // XCD-aware order: blocks b, b+8, b+16, ... share an XCD (round-robin dispatch), so give each XCD a
    // contiguous range of tiles = as few members (weight sets) as possible per private L2.
    const int T = (int)out.size();
    std::vector<Tile6> perm(T);
    const int qd = T / 8, rm = T % 8;
    for (int b = 0; b < T; ++b) {
        const int xcd = b % 8, slot = b / 8;
        const int base = xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd;
        perm[b] = out[base + slot];
    }
    out.swap(perm);
}

// ---- tile-size choice ------------------------------------------------------------------------------------------------
// A tile is 16*rc rows of one member; a CU keeps as many workgroups resident as their registers allow.  fp32 MFMA and
// VALU work add up on a SIMD whichever wave they come from, so a co-resident workgroup cannot hide arithmetic — but it
// does hide the stalls (barrier skew, LDS and L2 latency at the stage boundaries).  Cost of one 16-row chunk for the whole
// horizon in ms at H = 30 on MI355X, measured with exactly m tiles per CU (scripts/sweep_chunk_costs.py, round 3 with the
// rotating issue priority: profiles/r03_chunk_costs.jsonl): kChunkStart[nfw][rc][k-1] when k tiles start together on a CU and all
// stay resident (k up to the residency), kChunkNext[nfw][rc] for every further tile the dispatcher starts as an earlier one
// retires (fitted to m = 6 and to the BASELINE-config sweeps: B3 32, B5 10, B4 8 chunks per CU).  Co-resident tiles now advance
// together and retire together, so ONE tile more than the residency runs its whole horizon alone: it costs a round of two.
// Larger tiles re-use each streamed weight group for more rows; smaller ones pack the CUs more evenly and co-reside more easily.
// The constants are GENERATED from a sweep by fixed rules (scripts/sweep_chunk_costs.py --emit-table): regenerate them for another device
// or after a kernel change; tests/test_gpu_tileplan.py bounds how far the resulting automatic choice may be from the best forced one.
#include "cem_tile_costs.inc"
#define CEM_MAX_DEVICES 64
// workgroups of a <rc, nfw> tile one CU keeps resident, from the kernels' VGPR counts (512 registers per SIMD lane; round 3:
// plain kernel 139/159/186/218, 165/217/253/288; segment kernel 144/163/190/223, 171/221/255/292; round 4, with the sampler as the tiles'
// prologue: 153/161/189/222, 167/219/243/293 and 157/163/190/223, 172/222/255/294), [form][nfw - 1][rc - 1]
static const int kResidentStatic[2][2][4] = {{{4, 3, 2, 2}, {3, 2, 2, 1}}, {{3, 3, 2, 2}, {3, 2, 2, 1}}};

// The tuned rollout kernels exist for <chunks per tile 1 .. 4, input blocks per wave 1 .. 2>.  The one place a run-time (rc, nfw) picks
// the instantiation: fn(std::integral_constant<int, rc>, std::integral_constant<int, nfw>), or `none` for a pair outside the table.
template <class Ret, class Fn>
Ret with_tile_shape(int rc, int nfw, Ret none, Fn fn)
{
#define CEM_CASE(R, F) if (rc == R && nfw == F) return fn(std::integral_constant<int, R>{}, std::integral_constant<int, F>{});
    CEM_CASE(1, 1) CEM_CASE(2, 1) CEM_CASE(3, 1) CEM_CASE(4, 1)
    CEM_CASE(1, 2) CEM_CASE(2, 2) CEM_CASE(3, 2) CEM_CASE(4, 2)
#undef CEM_CASE
    return none;
}

template <int RC, int NFW>
int query_resident(bool seg)
{
    int n = 0;
    const size_t lds = CEM_ROLLOUT_LDS_BYTES(RC);
    const hipError_t e = seg ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cem_rollout_seg_kernel<RC, NFW>, 256, lds)
                             : hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, cem_rollout_kernel<RC, NFW, 0>, 256, lds);
    if (e != hipSuccess || n < 1) { (void)hipGetLastError(); return 0; }
    return n;
}

// Per-device facts the tile plan is priced with, asked from the runtime once per device (thread-safe: one std::call_once per
// device slot; the last slot serves a process without a device and holds the static tables).
struct DeviceFacts { std::once_flag once; int resident[2][2][4]; int cus; int cus_real; };
static DeviceFacts g_facts[CEM_MAX_DEVICES + 1];

const DeviceFacts &device_facts()
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = CEM_MAX_DEVICES; }     // no device: the static table's slot
    if (dev < 0 || dev > CEM_MAX_DEVICES) dev = CEM_MAX_DEVICES;
    DeviceFacts &f = g_facts[dev];
    std::call_once(f.once, [&] {
        const bool have = dev < CEM_MAX_DEVICES;
        for (int seg = 0; seg < 2; ++seg)
            for (int nfw = 1; nfw <= 2; ++nfw)
                for (int rc = 1; rc <= 4; ++rc) {
                    const int n = have ? with_tile_shape(rc, nfw, 0, [&](auto R, auto F) { return query_resident<R(), F()>(seg != 0); }) : 0;
                    f.resident[seg][nfw - 1][rc - 1] = n > 0 ? n : kResidentStatic[seg][nfw - 1][rc - 1];
                }
        f.cus = 256;                                // MI355X; a partitioned or different device reports its own count
        hipDeviceProp_t pr;
        if (have && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0) f.cus = pr.multiProcessorCount;
        else (void)hipGetLastError();
        // The cost model is per CU (tiles on the busiest CU x the cost of a chunk among k co-resident ones): another CU count only
        // changes how many tiles a CU gets, not the table.  CEM_ASSUME_CUS=n prices plans for n CUs (a diagnostic: the GPU-less host
        // helpers and tests/test_capi_cpu.py use it to see the choice move with the CU count).  It moves the tile PLAN only: whatever
        // has to hold on the device that runs the plan — how many workgroups are resident at once (the fused select's grid barriers, where
        // the sampler runs) — is computed from the real count, cus_real.
        f.cus_real = f.cus;
        if (const char *e = std::getenv("CEM_ASSUME_CUS")) { const int n = std::atoi(e); if (n >= 1 && n <= 4096) f.cus = n; }
    });
    return f;
}

// seg: the pinned + floating-segment launch (cem_rollout_seg_kernel) instead of one workgroup per tile (cem_rollout_kernel)
int resident_workgroups(int nfw, int rc, bool seg = false) { return device_facts().resident[seg ? 1 : 0][nfw - 1][rc - 1]; }
int num_cus() { return device_facts().cus; }            // what tile plans are priced for (CEM_ASSUME_CUS moves it)
int real_cus() { return device_facts().cus_real; }      // what the device has

// ---- pinned tiles + floating horizon segments ----------------------------------------------------------------------------
// One workgroup per tile for the whole horizon makes the busiest CU carry ceil(tiles / CUs) tiles while the mean is
// tiles / CUs (B2: 3 vs 2.44).  When every tile is resident at once that ratio is lost outright.  cem_rollout_seg_kernel gets
// most of it back: floor(tiles / CUs) tiles per CU stay whole ("pinned"), the remainder "float" — cut into S horizon segments
// that run, at raised priority, in whatever slot is free, so every CU carries about the same share of them.
// Measured on MI355X (scripts/sweep_seg.py, profiles/r02_sweep_floating_segments.jsonl): B2 0.475 -> 0.405 ms with S = 4..15;
// no gain with ONE pinned tile per CU (375 / 470 tiles: 0.335 -> 0.335, 0.353 -> 0.373 ms: the pinned tile runs without a
// partner and a floater's 30-step chain plus its hand-overs is as long as two whole tiles) and none when the remainder nearly
// fills the CUs anyway (750 tiles: 0.498 -> 0.492).  Hence: at least two pinned tiles per CU, and a predicted gain of > 4 %.
static const int kSegMaxSegments = 6, kSegMinSteps = 5;
// kFloatFactor (cem_tile_costs.inc): pinned + floating launch vs (mean tiles per CU) x the all-resident chunk cost, measured at B2

// cost of `per_cu` tiles of rc chunks queued on the BUSIEST CU, which keeps `occ` resident; `fill` = mean tiles per CU / per_cu <= 1.
// Co-resident tiles are priced by a sweep in which EVERY CU carries them; when only some do (fill < 1), the chip as a whole streams
// fewer weight groups through L2 and the doubly / triply loaded CUs finish earlier than that sweep says (375 one-chunk tiles: 0.305 ms
// against 2 x kChunkStart[0][0][1] = 0.335): kPartialFill, measured by the same sweep at 1.5 tiles per CU, scales that back.
double cu_cost(int nfw, int rc, long per_cu, int occ, double fill)
{
    const long k = std::min<long>(per_cu, occ);                             // tiles that start together (the table has three columns: a fourth co-resident tile is priced like the third)
    if (k < 1) return 0.0;
    const long later = per_cu - k + (per_cu == k + 1 && k > 1 ? 1 : 0);    // one tile beyond the residency: as dear as two (see above)
    const double relief = k >= 2 ? 1.0 - kPartialFill * (1.0 - std::min(std::max(fill, 0.0), 1.0)) : 1.0;
    return (double)rc * ((double)k * kChunkStart[nfw - 1][rc - 1][std::min<long>(k, 3) - 1] * relief + (double)later * kChunkNext[nfw - 1][rc - 1]);
}

int segments_for(const Dims &d, int rc, size_t n_tiles, int requested)
{
    if (requested == 1 || n_tiles >= (size_t)1 << 23) return 1;       // items are packed as (tile << 8 | segment)
    auto clamp_to_horizon = [&](int S) { S = std::min(S, d.H); while (S > 1 && (d.H + S - 1) / S * (S - 1) >= d.H) --S; return std::max(S, 1); };
    if (requested > 1) return clamp_to_horizon(requested);
    const int occ = resident_workgroups(d.NFW, rc, true), kNumCUs = num_cus();
    if (n_tiles < (size_t)2 * kNumCUs || n_tiles > (size_t)kNumCUs * occ) return 1;  // < 2 pinned tiles per CU: no gain (measured);
                                                                                  // more tiles than slots: the dispatcher already refills
    const int S = clamp_to_horizon(std::min(kSegMaxSegments, d.H / kSegMinSteps));
    if (S < 2) return 1;
    const double L = (double)n_tiles / kNumCUs;
    const long per_cu = (long)std::ceil(L);
    const double plain = cu_cost(d.NFW, rc, per_cu, occ, L / (double)per_cu), floating = (double)rc * L * kChunkStart[d.NFW - 1][rc - 1][std::min<long>(per_cu, 3) - 1] * kFloatFactor;
    return plain / floating > 1.10 ? S : 1;      // (a remainder that nearly fills the CUs gains nothing: 750 tiles measured 0.498 -> 0.492 ms in round 2)
}

double tile_plan_cost(const Dims &d, int rc, size_t n_tiles, int requested_segments)
{
    const int kNumCUs = num_cus();
    const int S = segments_for(d, rc, n_tiles, requested_segments);
    const double L = (double)n_tiles / kNumCUs;
    const long per_cu = (long)((n_tiles + kNumCUs - 1) / kNumCUs);
    if (S > 1 && n_tiles > (size_t)kNumCUs) {     // pinned tiles + floating segments: every CU carries the mean load
        if (n_tiles < (size_t)2 * kNumCUs)        // ONE pinned tile per CU runs without a partner and the floaters' chains set the time
            return (double)rc * L * kChunkStart[d.NFW - 1][rc - 1][0] * 1.35;       // (B2 at rc 2: 0.53 ms for 1.23 x 2 chunks per CU, round 3)
        return (double)rc * L * kChunkStart[d.NFW - 1][rc - 1][std::min<long>(per_cu, 3) - 1] * kFloatFactor;
    }
    return cu_cost(d.NFW, rc, per_cu, resident_workgroups(d.NFW, rc, false), per_cu > 0 ? L / (double)per_cu : 1.0);
}

// problems > 1: a batch handle's launch carries that many problems' tiles, and is priced for all of them
int auto_chunks(const Dims &d, int requested_segments, int problems = 1)
{
    int best = 1; double bestc = 1e30;
    for (int rc = 1; rc <= 4; ++rc) {
        std::vector<Tile6> t; build_plan_tiles(d, rc, t);
        const double cost = tile_plan_cost(d, rc, (size_t)problems * t.size(), requested_segments);
        // rc ascends: a cost within 0.5 % of the best so far goes to the larger tile (fewer workgroups, less weight traffic)
        if (cost <= bestc * 1.005) { best = rc; bestc = std::min(bestc, cost); }
    }
    return best;
}

// Tile size of the split-product rollout (cem_rollout_split.h).  It streams 1.5x the weight bytes at 2.7x the matrix rate, so one-chunk
// tiles are bound by the L2 -> CU path and larger tiles pay; what decides between the sizes is how many tiles the busiest CU gets
// (ceil(tiles / CUs)) and how many of them run side by side.  K cycles per step of ONE CU running m co-resident tiles of rc chunks,
// measured over population sizes (scripts/sweep_split_tiles.py, profiles/r03_split_tile_sizes.txt); residency: registers / LDS.
static const double kSplitStep[2][4][4] = {{{11.2, 18.2, 28.5, 0}, {15.8, 25.0, 0, 0}, {21.6, 34.2, 0, 0}, {27.2, 0, 0, 0}},
                                           {{14.2, 26.0, 0, 0}, {21.0, 39.0, 0, 0}, {28.5, 0, 0, 0}, {36.4, 0, 0, 0}}};
static const int kSplitResident[2][4] = {{3, 2, 2, 1}, {2, 2, 1, 1}};

// Tile size of the bf16 rollout (cem_rollout_bf16.h): the split kernel's rule on a table of its own.  A third of the split kernel's
// weight bytes and a sixth of its MFMAs per chunk; what decides between the sizes is again how many tiles the busiest CU gets
// (ceil(tiles / CUs)) and how many of them run side by side.  Plan ms (5 iterations, H = 30) of a device whose busiest CU runs m
// co-resident tiles of rc chunks, measured over population sizes (scripts/sweep_bf16_tiles.py, profiles/bf16_tile_sizes.txt: the rule
// picks the fastest size in 15 of its 16 rows and one 0.6 % behind in the other); only the ratios matter.  Residency: registers (512 / VGPRs of the planning instantiations:
// 113 145 171 205 | 155 185 221 253), LDS never binds.
static const double kBf16Step[2][4][4] = {{{0.45, 0.61, 0.82, 1.07}, {0.52, 0.70, 0.935, 0}, {0.61, 0.84, 0, 0}, {0.73, 0.985, 0, 0}},
                                          {{0.62, 0.865, 1.187, 0}, {0.79, 1.075, 0, 0}, {0.97, 1.35, 0, 0}, {1.17, 1.67, 0, 0}}};
static const int kBf16Resident[2][4] = {{4, 3, 2, 2}, {3, 2, 2, 2}};

// The one rule over either table: step[NFW - 1][rc - 1][m - 1] (zero past the residency R; the rule never reads past R - 1), the
// residency, and the tie margin — rc ascends, and within the margin the larger tile wins (fewer workgroups, less weight traffic: 5 % for
// the split kernel, whose larger tiles save a third or half of it, 2 % for the bf16 kernel).
struct ChunkedTileRule { const double (*step)[4][4]; const int (*resident)[4]; double tie; };
int auto_chunks_chunked(const Dims &d)
{
    const ChunkedTileRule rule = d.split() ? ChunkedTileRule{kSplitStep, kSplitResident, 1.05} : ChunkedTileRule{kBf16Step, kBf16Resident, 1.02};
    int best = 1; double bestc = 1e30;
    for (int rc = 1; rc <= 4; ++rc) {
        std::vector<Tile6> t; build_plan_tiles(d, rc, t);
        const long per_cu = (long)((t.size() + num_cus() - 1) / num_cus());
        const int R = rule.resident[d.NFW - 1][rc - 1];
        const double *ts = rule.step[d.NFW - 1][rc - 1];
        const double cost = (double)(per_cu / R) * ts[R - 1] + (per_cu % R ? ts[per_cu % R - 1] : 0.0);
        if (cost <= bestc * rule.tie) { best = rc; bestc = std::min(bestc, cost); }
    }
    return best;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Layout {
    size_t ctrl, musig, act_bounds, scores_local, scores_global, actions, act_pad, elite, returns, costs, result, wpack, bias_h, bias_mu, bias_var,
        nmin, ndelta, omask, kind_sel, etab, tiles, eps_out, stamps, seg_queue, seg_flags, seg_state,
        ms_hist, ms_sel, ms_counts, ms_best_sc, ms_best_ix, ms_part, ms_colmean, carry, expl, total;
};

struct Plan { int rc, n_tiles, n_seg, seg_len, n_pinned; };

// tile size, tile count and horizon segments of a configuration: one function, so workspace_bytes / create / the host helpers agree.
// mb > 0: the plan of a batch handle of mb problems (validate_batch: fp32 products on the tuned kernel) — the same tile-size rule priced
// for ALL mb problems' tiles in one launch (the results do not depend on the tile size), one workgroup per tile for the whole horizon (no
// floating segments: the work queue is per launch, not per problem; bit-identical either way).  n_tiles stays the count of ONE problem.
Plan make_plan(const cem_config_t *c, const Dims &d, int mb = 0)
{
    Plan pl{};
    const int seg_req = mb > 0 ? 1 : c->rollout_segments;
    pl.rc = d.wide ? 1 : (c->chunks_per_tile ? c->chunks_per_tile : auto_chunks(d, seg_req, std::max(mb, 1)));   // the wide kernel: 16-row tiles
    if (d.chunked() && !c->chunks_per_tile) pl.rc = auto_chunks_chunked(d);
    std::vector<Tile6> t; build_plan_tiles(d, pl.rc, t);
    pl.n_tiles = (int)t.size();
    pl.n_seg = (d.wide || d.chunked()) ? 1 : segments_for(d, pl.rc, t.size(), seg_req);
    pl.seg_len = (d.H + pl.n_seg - 1) / pl.n_seg;
    pl.n_seg = (d.H + pl.seg_len - 1) / pl.seg_len;
    // tiles every CU gets the same number of stay whole ("pinned"); only the remainder floats in segments
    pl.n_pinned = pl.n_seg > 1 ? (pl.n_tiles / num_cus()) * num_cus() : pl.n_tiles;
    if (c->rollout_segments > 1 && pl.n_pinned == pl.n_tiles && pl.n_seg > 1) pl.n_pinned = 0;   // an explicit request floats everything
    return pl;
}

// mb > 0: a batch handle of mb problems (cem_batch_planner_create) — every per-problem array becomes [mb] consecutive slices of the
// single-plan size (the kernels address problem b's slice from that size, cem_device.h RolloutParams::tiles_per_problem)
Layout make_layout(const cem_config_t *c, const Dims &d, size_t max_tiles, int mb = 0)
{
    Layout l{}; size_t o = 0;
    const size_t nb = mb > 0 ? (size_t)mb : 1;
    auto take = [&](size_t bytes) { size_t r = o; o = align256(o + bytes); return r; };
    l.ctrl = take(nb * sizeof(CtrlBlock));
    l.musig = take(nb * 2 * d.H * d.A * 4);
    l.act_bounds = take(64 * 4);
    l.scores_local = take(nb * d.Nloc * 4);
    l.scores_global = d.W > 1 ? take((size_t)d.N * 4) : l.scores_local;
    l.actions = take(nb * d.N * d.H * d.A * 4);
    l.act_pad = take(nb * d.N * d.H * d.act_nq * 16);
    l.elite = take(nb * d.k * 4);
    l.returns = take(nb * d.Bloc * 4);
    l.costs = take(nb * d.H * d.Bloc);
    l.result = take(mb > 0 ? nb * CEM_RESULT_WORDS * 4 : 64 * 4);
    l.wpack = take(d.wide ? (size_t)d.E * (align256(d.nat_member_floats * 4) + wide_image_floats(d) * 4) : (size_t)d.E * d.member_stride_f4 * 16);   // wide: natural blobs, then the packed images
    l.bias_h = take((size_t)d.E * d.L * CEM_U * 4);
    l.bias_mu = take((size_t)d.E * CEM_U * 4);
    l.bias_var = take((size_t)d.E * CEM_U * 4);
    l.nmin = take(CEM_U * 4);
    l.ndelta = take(CEM_U * 4);
    l.omask = take(2 * CEM_U * 4);
    l.kind_sel = take(CEM_NKIND * CEM_U * 4);
    l.etab = take((size_t)d.E * etab_rows(d) * CEM_U * 4);
    l.tiles = take(max_tiles * sizeof(TileDesc));
    l.eps_out = take(nb * CEM_MAX_ACT * 4);
    l.stamps = take(std::max<size_t>(max_tiles * 4 * 8, 128) * sizeof(long long));      // [tiles][4][8] rollout stamps; [64..71] select stamps
    // the SINGLE plan, for a batch handle too (which never floats a tile and would get the two minimum sizes): the size of these two
    // arrays decides every later offset, and batch workspaces keep the offsets they were introduced with
    const Plan pl = make_plan(c, d);
    l.seg_queue = take(256);
    const size_t n_float = (size_t)(pl.n_tiles - pl.n_pinned);
    l.seg_flags = take(std::max<size_t>(n_float * std::max(pl.n_seg - 1, 1), 1) * 4);
    l.seg_state = take(pl.n_seg > 1 ? std::max<size_t>(n_float, 1) * (2 * d.NFW * pl.rc * 256 + 64) * 16 : 16);
    // multi-workgroup select (large populations): digit histograms, per-slice counts and best elites, moment partial sums
    const size_t msG = ((size_t)d.N + CEM_MS_KEYS - 1) / CEM_MS_KEYS, msG2 = ((size_t)d.k + CEM_MS_EPG - 1) / CEM_MS_EPG;
    l.ms_hist = take(3 * CEM_MS_BINS * 4); l.ms_sel = take(256);
    l.ms_counts = take(msG * 2 * 4); l.ms_best_sc = take(msG * 4); l.ms_best_ix = take(msG * 4);
    l.ms_part = take(2 * msG2 * (size_t)d.H * d.A * 4); l.ms_colmean = take((size_t)d.H * d.A * 4);
    // warm start, behind everything else so that no earlier offset moves: per slot the carry (mu, sigma [H][A] of its last completed plan)
    // and the explicit initial distribution (cem_planner_set_initial_distribution)
    l.carry = take(nb * 2 * d.H * d.A * 4); l.expl = take(nb * 2 * d.H * d.A * 4);
    l.total = o;
    return l;
}

size_t max_tiles_of(const Dims &d) { std::vector<Tile6> t; build_plan_tiles(d, 1, t); return t.size(); }

// ---- batch handles (cem_batch_planner_create) ----------------------------------------------------------------------------
// What a batch handle serves (cem_mpc.h, the table at cem_batch_planner_create): one rank, fp32 products on the tuned rollout kernel,
// the one-workgroup select — every kernel of that path takes the problem from its grid and its own slices from the problem.
int validate_batch(const cem_config_t *c, int32_t mb)
{
    const int st = validate(c); if (st) return st;
    if (mb < 1 || mb > CEM_MAX_BATCH) return CEM_ERR_INVALID_ARG;
    if (c->world_size > 1 || c->precision != CEM_PRECISION_FP32) return CEM_ERR_UNSUPPORTED;
    const Dims d = make_dims(c);
    if (d.wide) return CEM_ERR_UNSUPPORTED;                                     // units > 128, an activation other than relu
    if (c->select_mode == 2 || c->select_mode == 3) return CEM_ERR_UNSUPPORTED;
    if (resolve_select_mode(c->select_mode, d.N, d.k, (long long)d.H * d.A, 140 * 1024, true, nullptr) != 1) return CEM_ERR_UNSUPPORTED;
    if ((long long)mb * (long long)max_tiles_of(d) > 0x7fffffffll) return CEM_ERR_UNSUPPORTED;   // the rollout grid: problems x tiles
    return CEM_OK;
}

}  // namespace

// ---- RCCL, opened at run time: the library has no link-time dependency on it (single-GPU users never load it), and in a
// process that already holds an RCCL (torch bundles one under the same SONAME) dlopen returns THAT copy, not a second one.
namespace {
struct CemNcclId { char internal[CEM_COMM_ID_BYTES]; };
struct Rccl {
    void *lib = nullptr;
    int (*GetUniqueId)(CemNcclId *) = nullptr;
    int (*CommInitRank)(void **, int, CemNcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
};
Rccl *rccl()
{
    static Rccl r;
    static std::once_flag once;                      // two handles may ask at once (one per env thread)
    std::call_once(once, [] {
        // CEM_RCCL_LIBRARY: load THIS file instead (a site's own RCCL build; tests/fakes/libfake_rccl.so, the shared-memory
        // stand-in with which several ranks share a one-GPU box).  Set and not loadable: no fallback, the error says so.
        if (const char *over = std::getenv("CEM_RCCL_LIBRARY")) {
            r.lib = dlopen(over, RTLD_NOW | RTLD_LOCAL);
            if (!r.lib) std::fprintf(stderr, "cem_mpc: CEM_RCCL_LIBRARY=%s: %s\n", over, dlerror());
        } else {
            for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
                r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
                if (r.lib) break;
            }
        }
        if (r.lib) {
            r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(r.lib, "ncclGetUniqueId");
            r.CommInitRank = (decltype(r.CommInitRank))dlsym(r.lib, "ncclCommInitRank");
            r.CommDestroy = (decltype(r.CommDestroy))dlsym(r.lib, "ncclCommDestroy");
            r.AllGather = (decltype(r.AllGather))dlsym(r.lib, "ncclAllGather");
            r.CommCount = (decltype(r.CommCount))dlsym(r.lib, "ncclCommCount");     // optional: only cem_planner_comm_ranks needs it
            if (!r.GetUniqueId || !r.CommInitRank || !r.CommDestroy || !r.AllGather) r.lib = nullptr;
        }
        // an environment variable has just decided which code the product calls for its collectives: say so, once, either way
        if (const char *over = std::getenv("CEM_RCCL_LIBRARY"))
            std::fprintf(stderr, r.lib ? "cem_mpc: RCCL entry points bound from CEM_RCCL_LIBRARY=%s%s\n" : "cem_mpc: CEM_RCCL_LIBRARY=%s lacks a required entry point%s\n",
                         over, (r.lib && !r.CommCount) ? " (no ncclCommCount: cem_planner_comm_ranks unavailable)" : "");
    });
    return r.lib ? &r : nullptr;
}
const int kNcclFloat32 = 7;        // ncclDataType_t ncclFloat32 (rccl.h)
}  // namespace
#define NCCLCHK(x) do { int e_ = (x); if (e_ != 0) { g_last_hip = e_; return CEM_ERR_COMM; } } while (0)

// A host that loads this library BEFORE the HIP runtime that owns its device memory (torch's wheel carries its own libamdhip64) ends up
// with two runtimes in the process: pointers from one are foreign to the other and the first call fails with hipErrorNoDevice or worse
// (INTEGRATION.md section 2).  The Python binding avoids it by importing torch first; any other host gets told, once, at its first create.
namespace {
int count_hip_runtimes(struct dl_phdr_info *info, size_t, void *data)
{
    if (info->dlpi_name && std::strstr(info->dlpi_name, "libamdhip64")) {
        auto *v = static_cast<std::vector<std::string> *>(data);
        if (std::find(v->begin(), v->end(), std::string(info->dlpi_name)) == v->end()) v->push_back(info->dlpi_name);
    }
    return 0;
}
void warn_if_two_hip_runtimes()
{
    static std::once_flag once;
    std::call_once(once, [] {
        std::vector<std::string> libs;
        dl_iterate_phdr(count_hip_runtimes, &libs);
        if (libs.size() > 1) {
            std::fprintf(stderr, "cem_mpc: %zu HIP runtimes are loaded in this process:", libs.size());
            for (const auto &l : libs) std::fprintf(stderr, " %s", l.c_str());
            std::fprintf(stderr, "\ncem_mpc: device memory and streams of one are foreign to the other — load libcem_mpc_gfx950.so AFTER the runtime that owns them (INTEGRATION.md)\n");
        }
    });
}
}  // namespace

// What one iteration launches: the handle's own plan (create), or — under a population schedule — that of the n[it]-wide configuration
struct IterPlan {
    Dims d;                                  // make_dims of the configuration with n_samples = n[it]
    int rc, n_tiles, n_seg, seg_len, n_pinned;
    bool sample_in_rollout, lean_rollout;
    size_t tiles_off;                        // byte offset of its tile list in cem_planner::pop_dev; (size_t)-1: the workspace's list (n[it] == n_samples)
};

struct cem_planner {
    cem_config_t cfg;
    Dims d;
    Layout lay;
    char *ws;
    hipStream_t stream;
    bool own_stream;
    int rc;
    int n_tiles;
    int n_seg, seg_len, n_pinned;           // horizon segments of the floating tiles (1 = one workgroup per tile), tiles that stay whole
    bool have_weights;
    bool in_plan;
    bool sample_in_rollout;                  // the sampler runs as the rollout tiles' prologue (else: cem_sample_kernel in front of the rollout launch)
    bool lean_rollout;                       // plans without caller noise tensors run cem_rollout_lean.hip's kernels (lean_eligible)
    bool lean_branchy;                       // CEM_FORCE_ROLLOUT=lean_branchy at create: never the straight-line form (lean_form)
    bool select_bucket;                      // CEM_FORCE_SELECT=bucket at create: never the ranked form of the one-workgroup select (select_form_of)
    const float *eps_act, *eps_model;       // current plan's explicit noise (device) or null
    // pinned host staging
    CtrlBlock *h_ctrl;
    float *h_result;
    WarmCtl *h_warm; const WarmCtl *d_h_warm;  // warm-start control of the next plan (stage_warm), read by cem_init_kernel alone
    uint32_t plan_seq;                       // plans staged on this handle (CtrlBlock::seq)
    const CtrlBlock *d_h_ctrl; float *d_h_result;     // the same two blocks as the DEVICE addresses them (hipHostGetDevicePointer)
    // timing
    bool timing; std::vector<hipEvent_t> ev; float roll_ms, sel_ms, red_ms, samp_ms; int roll_n;
    std::vector<std::pair<int, int>> ev_kind;   // (event index of start, kind 0 rollout / 1 select / 2 reduce / 3 sampler launch)
    // graph
    hipGraph_t graph; hipGraphExec_t gexec; bool graph_ready;
    ScorerDev sc;                            // the scorer as configured: cem_scorer_reward / cem_scorer_cost
    ScorerDev sc_roll;                       // what the rollouts and cem_compute_objective score with: sc — on a CEM_VARIANT_COST handle with a goal
                                             // threshold of -inf, so that no row is ever done and the cost bytes are un-masked (cem_score.h)
    float alpha, beta;
    void *comm;                              // ncclComm_t of cem_planner_comm_init, or null (the host exchanges scores_local -> scores_global)
    int plans_since_comm;                    // the first plan after comm_init runs eagerly (RCCL sets itself up lazily), then the graph is captured
    bool graph_failed;                       // capture with the collective did not work on this stack: stay eager
    size_t sel_dyn_limit;                    // dynamic-LDS allowance of the select kernels on this handle's device
    bool ranked_ready;                       // cem_select_ranked_kernel is in the library and has the same allowance
    int fused_resident;                      // workgroups of cem_msel_fused_kernel the device keeps resident at once (occupancy x CUs)
    bool sel_zeroed;                         // the multi-workgroup select's histograms / barrier counter were cleared by this iteration's reduce kernel
    bool fuse_banned;                        // a grid barrier of the fused select expired on this handle once (recovered in-stream): select_mode 2 from then on
    bool inject_capture_fail;                // cem_planner_inject_fault kind 2: treat the next graph capture of cem_planner_plan as refused by the runtime
    uint32_t inject_next;                    // cem_planner_inject_fault: CtrlBlock::inject of the next plan
    // grow-only device scratch of the standalone ops (unfold_sequences tiles + returns, compute_objective returns + costs)
    char *scratch; size_t scratch_bytes;
    std::vector<float> h_etab;               // host copy of RolloutParams::etab ([E][CEM_ET_ROWS + L][128]); uploaded whole by create / set_weights; set_normaliser uploads its two rows
    PackDesc *pack_desc; uint32_t n_pack_desc;   // cem_pack.h's unit table of this shape, a device allocation of the handle's own (cem_planner_set_weights_dev)
    int batch;                               // problems of a batch handle (cem_batch_planner_create); 0: a single-state handle
    int n_states;                            // problems of the batched plan being enqueued / last run (the rest are staged as done)
    // warm start (cem_mpc.h): per carry slot [max(batch, 1)]
    cem_warm_start_t warm;                   // parameters of CEM_INIT_SHIFT
    std::vector<int32_t> slot_mode;          // cem_init_mode, sticky
    std::vector<uint8_t> carry_valid, have_expl;
    std::vector<int32_t> carry_at;           // problem index whose mu / sigma slice still holds the slot's carry (the next plan's first kernel saves it), or -1: it is in Layout::carry
    std::vector<int32_t> slot_of;            // problem b -> carry slot (cem_planner_set_carry_slots), a permutation of 0 .. batch - 1
    bool warm_save_skipped;                  // the staged plan overwrites the one slot's carry without a copy (stage_warm)
    int warm_staged;                       // problems of the plan whose warm control is staged and whose outcome finish_warm has not seen yet
    std::vector<float> h_expl;               // host copy of the explicit uploads [slots][2][HA]: the source of their stream-ordered copies
    PlanOptions opt;                         // what the option setters set (cem_plan_options.h; its `comm` is filled by options_of); the fields below are what those options own
    // cem_planner_set_constraint (cem_score.h)
    float *budget_dev;                       // a device allocation of the handle's own, made on first use: budgets [slots], then cstat [slots][Nloc]
    std::vector<float> h_budget;             // host copy of the budgets [slots]: the source of their stream-ordered copies
    float *cstat_obj; size_t cstat_obj_n;    // grow-only cstat of cem_compute_objective (its candidate count is the caller's)
    const float *last_cstat; int last_cstat_n, last_cstat_problems;   // the C array of the last constrained reduce: per problem [last_cstat_n]
    // cem_planner_set_refit (cem_refit_weighted.h)
    float refit_beta;                        // fl32(1 / opt.refit_tau), rounded once here
    float *refit_dev;                        // a device allocation of the handle's own, made on first use: the select's discarded blend [slots][2][HA], then ESS [slots][I]
    bool refit_ran;                          // a weighted select has been put on the stream (cem_planner_refit_stats)
    // cem_planner_set_action_noise (cem_noise_mix.h)
    // CEM_NOISE_WHITE: the samplers draw their own Philox normals; CEM_NOISE_MIXED: they read noise_eps, which
    // cem_mix_action_noise_kernel fills behind the plan's first kernel
    std::vector<float> h_mix, h_mix_t;       // M [H][H] as set, and transposed: the source of its stream-ordered upload
    float *noise_dev;                        // a device allocation of the handle's own, made on first use: M transposed [H][H] (padded to a quad), then eps
    float *noise_eps; size_t noise_floats;   // eps [slots][I][N][H][A] inside noise_dev, and its float count
    // cem_planner_set_elite_carry (cem_elite_carry.h)
    float *elite_dev;                        // a device allocation of the handle's own, made by the first enabling call: counts [slots] (int32, padded to
                                             // 256 bytes), then the stores [slots][n_keep][H][A]
    int elite_cap;                           // rows per slot the allocation has room for (grows with n_keep, never shrinks)
    bool elite_clear;                        // a plan call returned an error: the counts are zeroed in front of the next plan
    // cem_planner_set_population_schedule / cem_planner_set_mean_candidate (cem_population.h)
    std::vector<IterPlan> pop;               // [I] the plan of every iteration while a schedule is on (opt.pop: their sizes); empty: off, every iteration is the handle's own plan
    char *pop_dev;                           // a device allocation of the handle's own: the tile lists of the iterations with n[it] != n_samples, then
                                             // (only when some iteration needs more than the workspace holds) segment flags and hand-over state
    uint32_t *pop_seg_flags; f4 *pop_seg_state;   // where a scheduled plan's floating tiles keep those two: the workspace's, or inside pop_dev
    int pop_n_ready;                         // FIFO entries the plan's first kernel clears: the most any iteration uses
    // cem_planner_set_plan_readout (cem_plan_readout.h)
    uint32_t *readout_dev;                   // a device allocation of the handle's own, made by the first enabling call: [slots] blocks of
                                             // CEM_READOUT_WORDS(H, A, P) words (the population never enters the size)
    // cem_planner_set_task (cem_task_score.h; the three kinds share cem_task_tile.h)
    float *task_dev;                         // a device allocation of the handle's own, made by the first enabling call: the tables
                                             // [CEM_TASK_TABLES][CEM_U], then the trajectories [Bloc][H + 1][O] of the last rollout launch
    TaskParams task;                         // the task as set: tab, r2, reward_goal, clip, rho (task_launch fills in the rest)
    // cem_planner_set_task_tracking (cem_task_reference.h)
    uint32_t *track_dev;                     // a device allocation of the handle's own, one per enabling call: the clock block
                                             // [CEM_TASK_CLOCK_WORDS], then the reference table [ref_steps][CEM_U]
    TaskParams track;                        // the tracking task as set: tab, ref, clock, T, r2, reward_goal, clip, rho, kappa
    std::vector<uint32_t> h_clock;           // host copy of the clock block: the source of its stream-ordered copies
    // cem_planner_set_task_zones (cem_task_zones.h)
    uint32_t *zones_dev;                     // a device allocation of the handle's own, one per enabling call: the zone table, then what a
                                             // quadratic base task lacks of a tracking task: a clock block of zeros, the tables with q in qT's row, the row g
    TaskParams zones;                        // the task with its zones as set: the base task's tables and scalars, zones, n_zones
    std::vector<float> h_task_tab;           // host copy of the task's tables as set: what a quadratic base's zones build theirs from
    // cem_planner_set_task_outputs (cem_task_outputs.h)
    uint32_t *outs_dev;                      // a device allocation of the handle's own, one per enabling call: C, the outputs' tables and reference, an
                                             // empty zone table, then (as zones_dev) what a quadratic base task lacks of a tracking task
    TaskParams outs;                         // the task with its outputs as set and no zones: what cem_planner_set_task_zones builds on while outputs are in force
};

namespace {

// problems side by side on the handle = its carry slots: a single-state handle is a handle of ONE problem
int warm_slots(const cem_planner *h) { return h->batch ? h->batch : 1; }

// The plan iteration `it` launches, as the enqueue functions read it: the handle's own, or the scheduled iteration's (cem_population.h)
struct IterView {
    const Dims *d; int rc, n_tiles, n_seg, seg_len, n_pinned; bool sample_in_rollout, lean_rollout;
    const TileDesc *tiles; uint32_t *seg_flags; f4 *seg_state;
};
IterView iter_view(const cem_planner *h, int it)
{
    const Layout &l = h->lay;
    if (h->pop.empty())
        return IterView{&h->d, h->rc, h->n_tiles, h->n_seg, h->seg_len, h->n_pinned, h->sample_in_rollout, h->lean_rollout,
                        (const TileDesc *)(h->ws + l.tiles), (uint32_t *)(h->ws + l.seg_flags), (f4 *)(h->ws + l.seg_state)};
    const IterPlan &ip = h->pop[std::min(std::max(it, 0), h->d.I - 1)];
    return IterView{&ip.d, ip.rc, ip.n_tiles, ip.n_seg, ip.seg_len, ip.n_pinned, ip.sample_in_rollout, ip.lean_rollout,
                    ip.tiles_off == (size_t)-1 ? (const TileDesc *)(h->ws + l.tiles) : (const TileDesc *)(h->pop_dev + ip.tiles_off),
                    h->pop_seg_flags, h->pop_seg_state};
}

// Which form of the lean kernels a lean iteration launches: 2, the straight-line form (cem_rollout_lean_straight.hip), where the plan's
// facts are the ones that form is compiled for — the goal a lidar kind, at most one constrained cost kind, every wave's weight stream
// exactly the groups one step consumes (layer 0: 4, three hidden layers and, on the waves with an observation block, the heads: 8
// each); else 1, the branchy form (cem_rollout_lean.hip), which CEM_FORCE_ROLLOUT=lean_branchy at create keeps for every plan.
// (The objective is that form's template parameter: enqueue_rollout stores cost bytes exactly where it asks for the safe order.)
int lean_form(const cem_planner *h, int it)
{
    const Dims &d = *iter_view(h, it).d; const ScorerDev &sc = h->sc_roll;
    bool straight = launch_rollout_lean_straight != nullptr && !h->lean_branchy && !sc.goal_mode && sc.n_cost <= 1 && d.L == 4 && d.NFW == 1;
    for (int w = 0; w < 4; ++w) straight = straight && d.wave_groups[w] == 4 + 3 * CEM_NG + (w < d.KB_obs ? CEM_NG : 0);
    return straight ? 2 : 1;
}
// the two parts of the task allocation (cem_planner::task_dev)
size_t task_tab_floats() { return (size_t)CEM_TASK_TABLES * CEM_U; }
float *task_traj(const cem_planner *h) { return h->task_dev + task_tab_floats(); }
// the second part of the tracking allocation (cem_planner::track_dev)
float *track_ref(uint32_t *dev) { return reinterpret_cast<float *>(dev + CEM_TASK_CLOCK_WORDS); }
// the parts of the zones allocation (cem_planner::zones_dev), in words
constexpr size_t kZoneTableWords = (size_t)CEM_TASK_MAX_ZONES * CEM_TASK_ZONE_WORDS;
constexpr size_t kZoneClockAt = kZoneTableWords, kZoneTabAt = kZoneClockAt + CEM_TASK_CLOCK_WORDS;
constexpr size_t kZoneRefAt = kZoneTabAt + (size_t)CEM_TASK_TABLES * CEM_U, kZoneWords = kZoneRefAt + CEM_U;
// the parts of the outputs allocation (cem_planner::outs_dev), in words: C, the outputs' tables, then the zones allocation's layout (an
// empty zone table; a quadratic base's restatement), then the outputs' reference [ref_rows][CEM_TASK_MAX_OUTPUTS]
constexpr size_t kOutTabAt = (size_t)CEM_TASK_MAX_OUTPUTS * CEM_U, kOutZoneAt = kOutTabAt + (size_t)CEM_TASK_OUT_TABLES * CEM_TASK_MAX_OUTPUTS;
constexpr size_t kOutRefAt = kOutZoneAt + kZoneWords;
// The ONE scoring launch of the task in force, for a plan's rollout (enqueue_rollout) and for a caller's trajectories (cem_task_score):
// `io` carries what differs between the two (traj, actions, ctrl, ret, costs, rows, N, H, check_done), the handle everything else;
// `missing` is the status where the kind's or the zones' allocation is not there.  The kind picks the kernel, zones the third
// whatever the kind (cem_task_tile.h)
int task_launch(cem_planner *h, const TaskParams &io, int missing)
{
    const bool tracking = h->opt.task == CEM_TASK_TRACKING, zoned = h->opt.zones != 0, outs = h->opt.outputs != 0;
    if (tracking && !h->track_dev) return missing;
    if (zoned && !h->zones_dev) return missing;
    if (outs && !h->outs_dev) return missing;
    const Dims &d = h->d;
    TaskParams tp = zoned ? h->zones : outs ? h->outs : tracking ? h->track : h->task;
    tp.traj = io.traj; tp.actions = io.actions; tp.ctrl = io.ctrl; tp.ret = io.ret; tp.costs = io.costs;
    tp.rows = io.rows; tp.N = io.N; tp.H = io.H; tp.O = d.O; tp.A = d.A; tp.check_done = io.check_done;
    tp.variant = h->cfg.variant != CEM_VARIANT_CEM ? 1 : 0;
    // compute_mean_costs has no done mask (safe_cem_mpc.py:98-108): near is never true and the cost bytes are not masked by done
    if (h->cfg.variant == CEM_VARIANT_COST) tp.r2 = 0.f;
    HIPCHK((outs ? launch_task_outputs : zoned ? launch_task_zones : tracking ? launch_task_reference : launch_task_score)(tp, h->stream));
    return CEM_OK;
}
int32_t *elite_counts(const cem_planner *h) { return reinterpret_cast<int32_t *>(h->elite_dev); }
size_t elite_count_floats(const cem_planner *h) { return ((size_t)warm_slots(h) + 63) & ~(size_t)63; }
float *elite_store(const cem_planner *h) { return h->elite_dev + elite_count_floats(h); }

// The select form the handle's next iteration takes (resolve_select_mode): the fused form only while the device keeps all its
// ceil(N / 4096) workgroups resident at once and none of its grid barriers has expired on this handle.
// (N: the population the select ranks — the handle's, or a scheduled iteration's)
int select_mode_for(const cem_planner *h, int N, bool *cache = nullptr)
{
    const Dims &d = h->d;
    const bool can_fuse = (N + CEM_MS_KEYS - 1) / CEM_MS_KEYS <= h->fused_resident && !h->fuse_banned;
    return resolve_select_mode(h->cfg.select_mode, N, d.k, (long long)d.H * d.A, h->sel_dyn_limit, can_fuse, cache);
}
int select_mode_now(const cem_planner *h, bool *cache = nullptr) { return select_mode_for(h, h->d.N, cache); }
// Which form of the one-workgroup select serves a (mode, cache, N) on this handle (select_ranked_form): 1, cem_select_ranked_kernel, only
// where the library has it, the device granted it the select's dynamic LDS and CEM_FORCE_SELECT=bucket did not keep form 0 at create.
// A function of the handle's constants and of what select_mode_for returns: where that changes, the graph is dropped already.
int select_form_of(const cem_planner *h, int mode, bool cache, int N)
{
    if (!h->ranked_ready || h->select_bucket) return 0;
    return select_ranked_form(mode, cache, N, h->cfg.variant == CEM_VARIANT_CEM);
}

// the captured plan no longer describes what the handle would launch (or never came to be): the next graphable plan captures anew
void drop_graph(cem_planner *h)
{
    if (h->gexec) { hipGraphExecDestroy(h->gexec); h->gexec = nullptr; }
    if (h->graph) { hipGraphDestroy(h->graph); h->graph = nullptr; }
    h->graph_ready = false;
}

// What iteration `it` of a plan launches, decided here once: enqueue_rollout and enqueue_select branch on it, launches_of counts it,
// the report functions (cem_planner_rollout_path / _rollout_form / _iteration_plan / _launches_per_iteration) read it.
// own_noise: the plan call brought noise tensors of its own, which the lean kernels — they draw in place — cannot take.
struct LaunchRecipe {
    bool sampler_launch;                     // cem_sample_kernel in front of the rollout launch (else the rollout's tiles sample as their prologue)
    bool inject_elites, inject_mean;         // behind that sampler: the kept elites into the first rows, the clipped mean into the last
    int lean_form;                           // 0: the generic rollout kernels; 1 / 2: the lean kernels, branchy / straight-line form (lean_form)
    bool fold_reduce;                        // a whole plan's select forms the particle mean itself: no score launch
    int select_mode; bool select_cache;      // the select form (select_mode_for) and whether the one-workgroup kernel stages its keys in LDS
    int select_form;                         // 1: the one-workgroup select is cem_select_ranked_kernel (select_form_of)
    bool one_workgroup_only;                 // something below, or a schedule: admit() let it onto a one-workgroup select only
    bool weighted, keep_elites, track;       // behind the select: the weighted refit, carry-over's keep, the read-out's tracker
    bool task;                               // the rollout is the family's MODE 1 kernel writing the handle's trajectory buffer, cem_task_score_kernel behind it
};
LaunchRecipe recipe_of(const cem_planner *h, int it, bool own_noise)
{
    const IterView v = iter_view(h, it); const PlanOptions &o = h->opt;
    LaunchRecipe r{};
    // Elite carry-over overwrites rows of a sample that lies in HBM between two launches: while it is on, the sampler is a launch of its
    // own and the rollouts are the generic kernels that read it, whatever create chose (which n_keep = 0 restores) — and so does the
    // mean candidate, in the one iteration it is written in (cem_population.h)
    r.inject_elites = o.elite.n_keep != 0;   // (a plan's iteration 0 has nothing to take without across_plans: enqueue_rollout; counted all the same)
    r.inject_mean = o.mean_cand && it == h->d.I - 1;
    // The task scorer reads trajectories only the MODE 1 kernels write, and those read a sample that lies in memory (cem_task_score.h)
    r.task = o.task != 0;
    const bool rewritten = r.inject_elites || r.inject_mean || r.task;
    r.sampler_launch = !v.sample_in_rollout || rewritten;
    // (the handle's own mixed tensor stands in wherever the caller passed none: the lean kernels step aside for it as for any tensor)
    r.lean_form = v.lean_rollout && !rewritten && !own_noise && o.noise_kind != CEM_NOISE_MIXED ? lean_form(h, it) : 0;
    r.select_mode = select_mode_for(h, v.d->N, &r.select_cache);
    r.select_form = select_form_of(h, r.select_mode, r.select_cache, v.d->N);
    // one rank (the scores need no exchange), the CemMpc objective (no per-step Beta counts; what the select folds IS the mean), and a
    // population the one-workgroup select serves with its keys staged in LDS
    r.fold_reduce = h->d.W == 1 && !h->comm && h->cfg.variant == CEM_VARIANT_CEM && !o.tail_m && r.select_mode == 1 && r.select_cache;
    r.weighted = o.refit_kind == CEM_REFIT_SOFTMAX; r.keep_elites = o.elite.n_keep != 0; r.track = o.readout != 0;
    r.one_workgroup_only = r.weighted || r.keep_elites || r.track || !h->pop.empty();
    return r;
}

// launches of iteration `it` (cem_planner_launches_per_iteration's rule): a count of what its recipe says — the rollout, the sampler
// where it is a launch of its own with what it carries behind it, the score kernel unless the select folds it, the select's, what follows it
int launches_of(const cem_planner *h, int it)
{
    const LaunchRecipe r = recipe_of(h, it, false);
    return 1 + r.sampler_launch + r.inject_elites + r.inject_mean + !r.fold_reduce + (r.select_mode == 2 ? 8 : r.select_mode == 3 ? 2 : 1) +
           r.weighted + r.keep_elites + r.track + r.task;
}

// The handle's options as a setter takes them.  Whether there is a communicator is the one fact not kept in cem_planner::opt: `comm` says it
PlanOptions options_of(const cem_planner *h) { PlanOptions o = h->opt; o.comm = h->comm != nullptr; return o; }

// T = H * m * kinds of a budget plan stays below this, so that an infeasible score's encoding is exact (cem_f32_encode_infeasible)
constexpr long long kBudgetTotalLimit = 1ll << 23;

// What the option rules read off the handle (cem_plan_options.h), for the schedule `next` asks for
HandleFacts facts_of(const cem_planner *h, const PlanOptions &next)
{
    const Dims &d = h->d;
    HandleFacts f;
    f.W = d.W; f.batch = h->batch; f.variant = h->cfg.variant; f.N = d.N; f.k = d.k; f.H = d.H; f.A = d.A; f.I = d.I; f.P = d.P;
    f.select_mode = select_mode_now(h);
    for (int32_t n : next.pop) f.pop_select_mode.push_back(select_mode_for(h, n));
    f.tail_max_p = CEM_TAIL_MAX_P; f.budget_max_tail_p = CEM_BUDGET_MAX_TAIL_P; f.elite_max_k = CEM_ELITE_MAX_K; f.mix_max_h = CEM_MIX_MAX_H;
    f.readout_max_p = CEM_READOUT_MAX_P; f.max_cost_kinds = CEM_MAX_COST_KINDS; f.budget_total_limit = kBudgetTotalLimit;
    f.refit_lds_bytes = CEM_REFIT_LDS_BYTES(d.k, d.H * d.A); f.refit_lds_limit = h->sel_dyn_limit;
    f.can_mix = launch_mix_action_noise && prepare_mix_action_noise; f.can_carry = launch_elite_keep && launch_elite_inject;
    f.can_mean = launch_mean_candidate != nullptr; f.can_track = launch_plan_track != nullptr; f.can_task = launch_task_score != nullptr;
    if (next.task == CEM_TASK_TRACKING) f.can_task = f.can_task && launch_task_reference != nullptr;   // (the kind's own kernel: cem_task_reference.h)
    f.can_zones = launch_task_zones != nullptr;
    f.can_outputs = launch_task_outputs != nullptr;
    return f;
}
int admit_on(const cem_planner *h, const PlanOptions &next, PlanChange change = PLAN_CHANGE_OTHER) { return admit(facts_of(h, next), next, change); }

// A setter changes what a plan launches.  The caller has admitted `next` and prepared whatever it needs — nothing of the handle is
// touched yet, so a failure up to here leaves it as it was.  Then: wait for the stream — `always`, where an EAGER plan still draining
// behind its polled result may be using what `swap_in` replaces; else only for a captured plan — let the caller swap its new state in,
// drop the graph (the captured plan holds the other setting's launches) and take `next`.  A swap_in that fails has changed nothing:
// the handle keeps its options and its graph.
template <typename SwapIn>
int commit_launch_change(cem_planner *h, PlanOptions &next, bool always, SwapIn swap_in)
{
    if (always || h->graph_ready) HIPCHK(hipStreamSynchronize(h->stream));
    if (const int st = swap_in()) return st;
    drop_graph(h);
    h->opt = std::move(next);
    return CEM_OK;
}
int commit_launch_change(cem_planner *h, PlanOptions &next, bool always) { return commit_launch_change(h, next, always, [] { return (int)CEM_OK; }); }

// a device allocation that goes again unless it is released into the handle: "free what this call allocated, leave the handle as it was"
struct DevBlock {
    void *p = nullptr;
    DevBlock() = default;
    DevBlock(const DevBlock &) = delete; DevBlock &operator=(const DevBlock &) = delete;
    ~DevBlock() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T *release() { T *q = static_cast<T *>(p); p = nullptr; return q; }
};

// what every handle owns from create on: the three pinned blocks, its stream if it made one, itself
void release_handle(cem_planner *h)
{
    if (h->h_ctrl) hipHostFree(h->h_ctrl);
    if (h->h_result) hipHostFree(h->h_result);
    if (h->h_warm) hipHostFree(h->h_warm);
    if (h->pack_desc) hipFree(h->pack_desc);
    if (h->budget_dev) hipFree(h->budget_dev);
    if (h->refit_dev) hipFree(h->refit_dev);
    if (h->noise_dev) hipFree(h->noise_dev);
    if (h->elite_dev) hipFree(h->elite_dev);
    if (h->readout_dev) hipFree(h->readout_dev);
    if (h->task_dev) hipFree(h->task_dev);
    if (h->track_dev) hipFree(h->track_dev);
    if (h->zones_dev) hipFree(h->zones_dev);
    if (h->outs_dev) hipFree(h->outs_dev);
    if (h->pop_dev) hipFree(h->pop_dev);
    if (h->cstat_obj) hipFree(h->cstat_obj);
    if (h->own_stream) hipStreamDestroy(h->stream);
    delete h;
}

}  // namespace

extern "C" {

int cem_abi_version(void) { return CEM_ABI_VERSION; }
int cem_last_hip_error(void) { return g_last_hip; }

const char *cem_status_string(int s)
{
    switch (s) {
    case CEM_OK: return "ok";
    case CEM_ERR_INVALID_ARG: return "invalid argument";
    case CEM_ERR_UNSUPPORTED: return "unsupported configuration (units <= 256, obs+act <= 128, task 'goal')";
    case CEM_ERR_SPLIT: return "particles*n_samples is not divisible by ensemble_size (tf.split would raise)";
    case CEM_ERR_WORKSPACE: return "workspace too small or misaligned";
    case CEM_ERR_HIP: return "HIP runtime error (see cem_last_hip_error)";
    case CEM_ERR_NO_WEIGHTS: return "set_weights has not been called";
    case CEM_ERR_STATE: return "stepwise plan calls out of order, or a standalone call while a plan is in flight";
    case CEM_ERR_COMM: return "RCCL: library not found or a collective call failed (see cem_last_hip_error for the ncclResult_t)";
    case CEM_ERR_DEVICE: return "a kernel could not finish its work (a floating rollout segment starved of its work-queue entry, or an expired fused-select barrier whose recovery did not run): result not valid";
    default: return "unknown status";
    }
}

size_t cem_weight_blob_floats(const cem_config_t *cfg)
{
    if (validate(cfg) != CEM_OK) return 0;
    const Dims d = make_dims(cfg);
    return d.nat_member_floats * d.E;
}

size_t cem_packed_weight_floats(const cem_config_t *cfg)
{
    if (validate(cfg) != CEM_OK) return 0;
    const Dims d = make_dims(cfg);
    if (d.wide) return 0;                               // the wide kernel reads the natural blob: nothing is packed
    return (size_t)d.member_stride_f4 * 4 * d.E;
}

size_t cem_workspace_bytes(const cem_config_t *cfg)
{
    if (validate(cfg) != CEM_OK) return 0;
    const Dims d = make_dims(cfg);
    return make_layout(cfg, d, max_tiles_of(d)).total;
}

int cem_pack_weights_host(const cem_config_t *cfg, const float *blob, float *packed)
{
    int st = validate(cfg); if (st) return st;
    if (!blob || !packed) return CEM_ERR_INVALID_ARG;
    const Dims d = make_dims(cfg);
    if (d.wide) return CEM_ERR_UNSUPPORTED;
    for (int m = 0; m < d.E; ++m) {
        if (d.chunked()) pack_member_chunked(d, blob + (size_t)m * d.nat_member_floats, reinterpret_cast<uint16_t *>(packed + (size_t)m * d.member_stride_f4 * 4));
        else pack_member(d, blob + (size_t)m * d.nat_member_floats, packed + (size_t)m * d.member_stride_f4 * 4);
    }
    return CEM_OK;
}

int cem_plan_tiles_host(const cem_config_t *cfg, int32_t *rc_out, int32_t *n_tiles_out, int32_t *tiles_out, int32_t max_tiles)
{
    int st = validate(cfg); if (st) return st;
    const Dims d = make_dims(cfg);
    const int rc = make_plan(cfg, d).rc;
    std::vector<Tile6> t; build_plan_tiles(d, rc, t);
    if (rc_out) *rc_out = rc;
    if (n_tiles_out) *n_tiles_out = (int32_t)t.size();
    if (tiles_out) {
        if ((int)t.size() > max_tiles) return CEM_ERR_INVALID_ARG;
        std::memcpy(tiles_out, t.data(), t.size() * sizeof(Tile6));
    }
    return CEM_OK;
}

int cem_plan_segments_host(const cem_config_t *cfg, int32_t *segments_out, int32_t *steps_per_segment_out)
{
    int st = validate(cfg); if (st) return st;
    const Dims d = make_dims(cfg);
    const Plan pl = make_plan(cfg, d);
    if (segments_out) *segments_out = pl.n_seg;
    if (steps_per_segment_out) *steps_per_segment_out = pl.seg_len;
    return CEM_OK;
}

int cem_rollout_residency(int32_t chunks_per_tile, int32_t input_blocks_per_wave, int32_t *table_out, int32_t *runtime_out)
{
    // [0]: one workgroup per tile (cem_rollout_kernel), [1]: the pinned + floating-segment form (cem_rollout_seg_kernel)
    if (chunks_per_tile < 1 || chunks_per_tile > 4 || input_blocks_per_wave < 1 || input_blocks_per_wave > 2) return CEM_ERR_INVALID_ARG;
    for (int seg = 0; seg < 2; ++seg) {
        if (table_out) table_out[seg] = kResidentStatic[seg][input_blocks_per_wave - 1][chunks_per_tile - 1];
        if (runtime_out)
            runtime_out[seg] = with_tile_shape(chunks_per_tile, input_blocks_per_wave, 0, [&](auto R, auto F) { return query_resident<R(), F()>(seg != 0); });
    }
    return CEM_OK;
}

}  // extern "C"

// The lean one-chunk rollout (cem_rollout_lean.hip: actions drawn in the lanes whose model noise is discarded, no materialised sample)
// serves the one-chunk fp32 kernel of the obs + act <= 64 family with every feature quad all-observation or all-action, single-rank
// single-state plans whose tiles sample inside the rollout launch (all resident at once: B1, B2), and a horizon whose mu / sigma quads
// fit its LDS allowance.  Everything else — and any plan given explicit noise tensors — runs the generic kernels.
static bool lean_eligible(const cem_planner *h, const Dims &d, int rc, bool sample_in_rollout)
{
    return launch_rollout_lean != nullptr && !d.wide && !d.chunked() && rc == 1 && d.NFW == 1 && d.L == 4 && d.O % 4 == 0 && h->cfg.world_size == 1 && !h->batch &&
           sample_in_rollout && CEM_LEAN_ACT_LDS_BYTES(d.H, (d.A + 3) / 4) <= CEM_LEAN_ACT_LDS_MAX;
}

// Where the sampler runs (cem_device.h: cem_tile_sample_actions vs cem_sample_kernel) and which rollout kernels serve the plan `pl` of
// the shape `d` on this handle: create's rule, and — per iteration — the population schedule's.
// Inside the rollout launch when ALL its tiles are resident at once (one round of prologues per launch: B1, B2) — one launch and one
// graph node fewer per iteration for about what the launch cost; as a launch of its own when tiles queue for slots (B3: 8 tiles per CU;
// every round of tiles would pay the prologue on its critical path, and each candidate is sampled once per particle: K = 16 measured
// +1.5 % on the launch).
static void place_sampler(const cem_planner *h, const Dims &d, const Plan &pl, bool *sample_in_rollout, bool *lean_rollout)
{
    const size_t nb = (size_t)warm_slots(h);
    // (the bf16 kernel: one slot per CU, like the split kernel — its launch is short enough that a second co-resident tile's prologue,
    // which samples every candidate once per particle, shows: B4's 512 four-chunk tiles 2.70 ms per plan inside against 2.48 in a launch
    // of its own, the shipped safe shape 0.603 against 0.612, B2 inside either way; profiles/bf16_rollout_isa.txt)
    const int slots = real_cus() * ((d.wide || d.chunked()) ? 1 : resident_workgroups(d.NFW, pl.rc, pl.n_seg > 1));
    *sample_in_rollout = (long long)nb * pl.n_tiles <= slots;          // (a batch handle: all its problems' tiles in one launch)
    if (const char *e = std::getenv("CEM_FORCE_SAMPLER"))      // diagnostic / tests: "tile" or "kernel" — the results do not depend on it
        *sample_in_rollout = std::strcmp(e, "kernel") != 0;
    *lean_rollout = lean_eligible(h, d, pl.rc, *sample_in_rollout);
    if (const char *e = std::getenv("CEM_FORCE_ROLLOUT"))      // diagnostic / tests: "generic", "lean" or "lean_branchy" (planner_create) — the results do not depend on it; "lean" on an ineligible handle is ignored
        *lean_rollout = *lean_rollout && std::strcmp(e, "generic") != 0;
}

// mb = 0: a single-state handle (cem_planner_create); mb > 0: a batch handle of mb problems (cem_batch_planner_create)
static int planner_create(const cem_config_t *cfg, int32_t mb, void *workspace, size_t workspace_bytes, void *hip_stream, cem_planner_t **out)
{
    int st = mb ? validate_batch(cfg, mb) : validate(cfg); if (st) return st;
    if (!workspace || !out) return CEM_ERR_INVALID_ARG;
    if (cfg->precision == CEM_PRECISION_BF16 && (launch_rollout_bf16 == nullptr || launch_pack_bf16 == nullptr)) return CEM_ERR_UNSUPPORTED;   // a build without cem_rollout_bf16.hip
    warn_if_two_hip_runtimes();
    cem_planner *h = new (std::nothrow) cem_planner();
    if (!h) return CEM_ERR_INVALID_ARG;
    h->cfg = *cfg; h->d = make_dims(cfg);
    h->batch = mb; h->n_states = warm_slots(h);
    const size_t nb = (size_t)warm_slots(h);
    h->lay = make_layout(cfg, h->d, max_tiles_of(h->d), mb);
    if (workspace_bytes < h->lay.total || ((uintptr_t)workspace & 255)) { delete h; return CEM_ERR_WORKSPACE; }
    h->ws = (char *)workspace; h->stream = (hipStream_t)hip_stream; h->own_stream = false;
    if (!h->stream) {      // the legacy default stream cannot be captured into a hipGraph: use a stream of our own
        if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) { g_last_hip = (int)hipGetLastError(); delete h; return CEM_ERR_HIP; }
        h->own_stream = true;
    }
    { const Plan pl = make_plan(cfg, h->d, mb); h->rc = pl.rc; h->n_seg = pl.n_seg; h->seg_len = pl.seg_len; h->n_pinned = pl.n_pinned;
      place_sampler(h, h->d, pl, &h->sample_in_rollout, &h->lean_rollout); }
    { const char *e = std::getenv("CEM_FORCE_ROLLOUT"); h->lean_branchy = e && std::strcmp(e, "lean_branchy") == 0; }
    { const char *e = std::getenv("CEM_FORCE_SELECT"); h->select_bucket = e && std::strcmp(e, "bucket") == 0; }     // diagnostic / tests: the results do not depend on it
    h->have_weights = false; h->in_plan = false; h->eps_act = h->eps_model = nullptr;
    h->timing = false; h->roll_ms = h->sel_ms = h->red_ms = h->samp_ms = 0.f; h->roll_n = 0;
    h->graph = nullptr; h->gexec = nullptr; h->graph_ready = false;     // (h->opt: every option off, PlanOptions' own defaults)
    h->budget_dev = nullptr; h->cstat_obj = nullptr; h->cstat_obj_n = 0; h->last_cstat = nullptr; h->last_cstat_n = h->last_cstat_problems = 0;
    h->refit_beta = 0.f; h->refit_dev = nullptr; h->refit_ran = false;
    h->noise_dev = nullptr; h->noise_eps = nullptr; h->noise_floats = 0;
    h->elite_dev = nullptr; h->elite_cap = 0; h->elite_clear = false;
    h->readout_dev = nullptr;
    h->task_dev = nullptr; h->task = TaskParams{};
    h->track_dev = nullptr; h->track = TaskParams{}; h->h_clock.assign(CEM_TASK_CLOCK_WORDS, 0u);
    h->zones_dev = nullptr; h->zones = TaskParams{};
    h->outs_dev = nullptr; h->outs = TaskParams{};
    h->pop_dev = nullptr; h->pop_seg_flags = nullptr; h->pop_seg_state = nullptr; h->pop_n_ready = 0;
    h->h_budget.assign(nb, std::numeric_limits<float>::infinity());
    h->comm = nullptr; h->plans_since_comm = 0; h->graph_failed = false;
    h->h_ctrl = nullptr; h->h_result = nullptr; h->h_warm = nullptr; h->d_h_warm = nullptr; h->pack_desc = nullptr; h->n_pack_desc = 0;
    h->warm = cem_warm_start_t{}; h->warm.shift = 1; h->warm_staged = 0; h->warm_save_skipped = false;
    h->slot_mode.assign(nb, CEM_INIT_COLD); h->carry_valid.assign(nb, 0); h->have_expl.assign(nb, 0); h->carry_at.assign(nb, -1);
    h->slot_of.resize(nb); for (size_t b = 0; b < nb; ++b) h->slot_of[b] = (int32_t)b;
    h->h_expl.assign(nb * 2 * h->d.H * h->d.A, 0.f);
    h->scratch = nullptr; h->scratch_bytes = 0; h->sel_zeroed = false; h->plan_seq = 0; h->fuse_banned = false; h->inject_next = 0; h->inject_capture_fail = false;
    // every failure from here on frees what was acquired and reports the HIP code
    auto fail = [&](int status) { g_last_hip = (int)hipGetLastError(); release_handle(h); return status; };
    // mapped + coherent (fine-grained) host memory, asked for explicitly: the device reads the staged block and writes the result in place,
    // and the host polls that result while the stream is still running
    const size_t result_bytes = mb ? nb * CEM_RESULT_WORDS * 4 : 64 * 4;
    if (hipHostMalloc((void **)&h->h_ctrl, nb * sizeof(CtrlBlock), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc((void **)&h->h_result, result_bytes, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostMalloc((void **)&h->h_warm, sizeof(WarmCtl) + nb * sizeof(WarmProb), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) return fail(CEM_ERR_HIP);
    {   // the device packers' unit table (cem_pack.h): a function of the shape alone
        const std::vector<PackDesc> table = build_pack_table(h->d);
        h->n_pack_desc = (uint32_t)table.size();
        // the table must tile a member's image exactly: the pack kernels write one unit per descriptor (plus 4 KB of slack)
        const size_t image_bytes = h->d.wide ? wide_image_floats(h->d) * 4 : (size_t)h->d.member_stride_f4 * 16 - 4096;
        if (table.size() * (h->d.group_bytes() / 2) != image_bytes) return fail(CEM_ERR_STATE);      // (a group is two units: output blocks a, b)
        if (hipMalloc((void **)&h->pack_desc, table.size() * sizeof(PackDesc)) != hipSuccess ||
            hipMemcpy(h->pack_desc, table.data(), table.size() * sizeof(PackDesc), hipMemcpyHostToDevice) != hipSuccess) return fail(CEM_ERR_HIP);
    }
    std::memset(h->h_warm, 0, sizeof(WarmCtl) + nb * sizeof(WarmProb));
    std::memset(h->h_ctrl, 0, nb * sizeof(CtrlBlock));
    std::memset(h->h_result, 0, result_bytes);
    {   // kernels read the staged control block and write the plan's result in place (no copy nodes around a plan)
        void *dc = nullptr, *dr = nullptr, *dw = nullptr;
        if (hipHostGetDevicePointer(&dc, h->h_ctrl, 0) != hipSuccess || hipHostGetDevicePointer(&dr, h->h_result, 0) != hipSuccess ||
            hipHostGetDevicePointer(&dw, h->h_warm, 0) != hipSuccess) return fail(CEM_ERR_HIP);
        h->d_h_ctrl = (const CtrlBlock *)dc; h->d_h_result = (float *)dr; h->d_h_warm = (const WarmCtl *)dw;
    }
    auto upload = [&](size_t off, const void *src, size_t bytes) {
        return hipMemcpyAsync(h->ws + off, src, bytes, hipMemcpyHostToDevice, h->stream) == hipSuccess;
    };

    // scorer constants, rounded the way the reference's Python-float -> fp32 tensor conversion rounds them
    const cem_scorer_t &s = cfg->scorer;
    ScorerDev &sc = h->sc;
    sc.goal_mode = s.goal_mode; sc.goal_lo = s.goal_lo; sc.goal_hi = s.goal_hi; sc.D = s.lidar_max_dist;
    sc.goal_thresh = s.goal_reached_dist;        // fl32(0.8 * goal_size) evaluated in double by the caller (safety_gym.py:116)
    sc.reward_distance = s.reward_distance; sc.reward_goal = s.reward_goal; sc.reward_clip = s.reward_clip;
    sc.indicator = s.constrain_indicator; sc.n_cost = s.n_cost_kinds;
    for (int i = 0; i < 4; ++i) { sc.cost_lo[i] = s.cost_lo[i]; sc.cost_hi[i] = s.cost_hi[i]; sc.cost_size[i] = s.cost_size[i]; }
    h->sc_roll = sc;
    if (cfg->variant == CEM_VARIANT_COST) h->sc_roll.goal_thresh = -std::numeric_limits<float>::infinity();   // goal distances are >= 0: never reached
    {   // Beta prior of safe_cem_mpc.py:113-115 in fp32 tensor arithmetic (mu = 0.5, sigma = 0.27 from :81)
        const float mu = 0.5f, sg = 0.27f;
        const float alpha = (((1.0f - mu) / (sg * sg)) - 1.0f / mu) * (mu * mu);
        h->alpha = alpha; h->beta = alpha * (1.0f / mu - 1.0f);
    }

    // tiles, per-feature predicate tables of the rollout epilogue, identity normaliser (until set_normaliser) -> device
    std::vector<Tile6> tiles; build_plan_tiles(h->d, h->rc, tiles);
    h->n_tiles = (int)tiles.size();
    const Dims &d = h->d;
    std::vector<float> om(2 * CEM_U, 0.f), ks(CEM_NKIND * CEM_U, std::numeric_limits<float>::infinity());
    const float ninf = -std::numeric_limits<float>::infinity();
    for (int f = 0; f < CEM_U; ++f) {
        om[f] = f < d.O ? 1.f : 0.f;
        om[CEM_U + f] = (f >= d.O && f < d.O + d.A) ? 1.f : 0.f;
        const int ghi = s.goal_mode ? s.goal_lo + 1 : s.goal_hi;
        if (f >= s.goal_lo && f < ghi && f < d.O) ks[f] = ninf;
        for (int k = 0; k < s.n_cost_kinds; ++k)
            if (f >= s.cost_lo[k] && f < s.cost_hi[k] && f < d.O) ks[(k + 1) * CEM_U + f] = ninf;
    }
    std::vector<float> mn(CEM_U, 0.f), dl(CEM_U, 1.f);
    // the hot kernel's per-member table: identity normaliser and zero biases until set_normaliser / set_weights fill them in
    const size_t et_rows = etab_rows(d);
    h->h_etab.assign((size_t)d.E * et_rows * CEM_U, 0.f);
    for (int m = 0; m < d.E; ++m) {
        float *et = &h->h_etab[(size_t)m * et_rows * CEM_U];
        for (int f = 0; f < CEM_U; ++f) {
            et[CEM_ET_RDELTA * CEM_U + f] = 1.f;
            et[CEM_ET_OBS * CEM_U + f] = om[f]; et[CEM_ET_ACT * CEM_U + f] = om[CEM_U + f];
            et[CEM_ET_SEL0 * CEM_U + f] = ks[f]; et[CEM_ET_SEL1 * CEM_U + f] = ks[CEM_U + f];
        }
    }
    float bounds[64] = {0.f};                              // tf.clip_by_value's lb / ub (cem_mpc.py:48), read by the rollout tiles' sampling prologue
    for (int a = 0; a < d.A; ++a) { bounds[a] = cfg->act_lb[a]; bounds[32 + a] = cfg->act_ub[a]; }
    if (!upload(h->lay.act_bounds, bounds, sizeof(bounds)) ||
        !upload(h->lay.tiles, tiles.data(), tiles.size() * sizeof(Tile6)) || !upload(h->lay.omask, om.data(), om.size() * 4) ||
        !upload(h->lay.kind_sel, ks.data(), ks.size() * 4) || !upload(h->lay.nmin, mn.data(), CEM_U * 4) ||
        !upload(h->lay.ndelta, dl.data(), CEM_U * 4) || !upload(h->lay.etab, h->h_etab.data(), h->h_etab.size() * 4) ||
        hipMemsetAsync(h->ws + h->lay.act_pad, 0, nb * d.N * d.H * d.act_nq * 16, h->stream) != hipSuccess ||   // the padding words of the action quads are never written again
        hipStreamSynchronize(h->stream) != hipSuccess)
        return fail(CEM_ERR_HIP);

    // Select kernel: scores staged in LDS when they fit.  gfx950 has 160 KB per CU and this kernel is the CU's only workgroup;
    // beyond the default 64 KB per workgroup the runtime has to be asked, per device (19 KB of the budget are the kernel's
    // static arrays).  Both variants: the uncached one still keeps the elite list (up to 24576 indices = 96 KB) in dynamic LDS.
    h->sel_dyn_limit = 48 * 1024;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_select_kernel<true, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            140 * 1024) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_select_kernel<true, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            140 * 1024) == hipSuccess &&
        hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_select_kernel<false, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            140 * 1024) == hipSuccess) h->sel_dyn_limit = 140 * 1024;
    else (void)hipGetLastError();
    h->ranked_ready = launch_select_ranked && prepare_select_ranked && prepare_select_ranked(h->sel_dyn_limit) == hipSuccess;
    if (!h->ranked_ready) (void)hipGetLastError();
    {
        int per_cu = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, cem_msel_fused_kernel, 1024, 0) != hipSuccess || per_cu < 1) { (void)hipGetLastError(); per_cu = 0; }
        h->fused_resident = per_cu * real_cus();
    }
    // a batch handle runs the one-workgroup select only: on a device that grants less dynamic LDS than validate_batch() assumed, the
    // shape may need another form
    if (mb && select_mode_now(h) != 1) { release_handle(h); return CEM_ERR_UNSUPPORTED; }
    *out = h;
    return CEM_OK;
}

extern "C" {

int cem_planner_create(const cem_config_t *cfg, void *workspace, size_t workspace_bytes, void *hip_stream, cem_planner_t **out)
{
    return planner_create(cfg, 0, workspace, workspace_bytes, hip_stream, out);
}

size_t cem_batch_workspace_bytes(const cem_config_t *cfg, int32_t max_batch)
{
    if (validate_batch(cfg, max_batch) != CEM_OK) return 0;
    const Dims d = make_dims(cfg);
    return make_layout(cfg, d, max_tiles_of(d), max_batch).total;
}

int cem_batch_planner_create(const cem_config_t *cfg, int32_t max_batch, void *workspace, size_t workspace_bytes, void *hip_stream,
                             cem_planner_t **out)
{
    const int st = validate_batch(cfg, max_batch); if (st) return st;      // (max_batch 0 would be planner_create's single-state handle)
    return planner_create(cfg, max_batch, workspace, workspace_bytes, hip_stream, out);
}

int cem_planner_batch_capacity(const cem_planner_t *h, int32_t *max_batch_out)
{
    if (!h || !max_batch_out) return CEM_ERR_INVALID_ARG;
    *max_batch_out = h->batch;
    return CEM_OK;
}

int cem_planner_destroy(cem_planner_t *h)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    // a polled plan returns when its result block lands, which may be before the stream has drained (the graph's tail — e.g. the
    // early-exit kernels behind an early stop — still reads the workspace and the pinned blocks freed below)
    if (hipStreamSynchronize(h->stream) != hipSuccess) (void)hipGetLastError();
    if (h->scratch) hipFree(h->scratch);
    if (h->comm) { if (Rccl *r = rccl()) r->CommDestroy(h->comm); h->comm = nullptr; }
    drop_graph(h);
    for (auto e : h->ev) hipEventDestroy(e);
    release_handle(h);
    return CEM_OK;
}

int cem_planner_layout(const cem_planner_t *h, cem_layout_t *o)
{
    if (!h || !o) return CEM_ERR_INVALID_ARG;
    o->scores_local = h->lay.scores_local; o->scores_global = h->lay.scores_global; o->actions = h->lay.actions;
    o->mu_sigma = h->lay.musig; o->elite_idx = h->lay.elite; o->returns = h->lay.returns; o->costs = h->lay.costs;
    o->result = h->lay.result; o->stamps = h->lay.stamps; o->total = h->lay.total;
    o->wpack = h->lay.wpack; o->wpack_bytes = h->d.wide ? align256(h->d.nat_member_floats * h->d.E * 4) + wide_image_floats(h->d) * 4 * h->d.E : (size_t)h->d.E * h->d.member_stride_f4 * 16; o->bias_h = h->lay.bias_h; o->bias_mu = h->lay.bias_mu; o->bias_var = h->lay.bias_var;
    o->etab = h->lay.etab; o->etab_bytes = (size_t)h->d.E * etab_rows(h->d) * CEM_U * 4;
    return CEM_OK;
}

int cem_planner_set_weights(cem_planner_t *h, const float *blob, size_t n_floats)
{
    if (!h || !blob) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    if (n_floats != d.nat_member_floats * d.E) return CEM_ERR_INVALID_ARG;
    if (d.wide) {                                       // the wide kernel: natural blobs (biases) + per-member operand-order images
        const size_t img = wide_image_floats(d);
        std::vector<float> images(img * d.E);
        for (int m = 0; m < d.E; ++m) pack_member_wide(d, blob + (size_t)m * d.nat_member_floats, images.data() + (size_t)m * img);
        HIPCHK(hipMemcpyAsync(h->ws + h->lay.wpack, blob, n_floats * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipMemcpyAsync(h->ws + h->lay.wpack + align256(n_floats * 4), images.data(), images.size() * 4, hipMemcpyHostToDevice, h->stream));
        const NatOff no = nat_offsets(d);                // the biases as rows of the per-member table (hidden layers: 256 features = 2 rows)
        const size_t et_rows = etab_rows(d);
        for (int m = 0; m < d.E; ++m) {
            const float *nat = blob + (size_t)m * d.nat_member_floats;
            float *et = &h->h_etab[(size_t)m * et_rows * CEM_U];
            std::memset(et + CEM_ET_BMU * CEM_U, 0, 2 * CEM_U * 4);
            std::memcpy(et + CEM_ET_BMU * CEM_U, nat + no.bmu, d.O * 4);
            std::memcpy(et + CEM_ET_BVAR * CEM_U, nat + no.bvar, d.O * 4);
            std::memset(et + CEM_ET_ROWS * CEM_U, 0, (size_t)2 * d.L * CEM_U * 4);
            for (int l = 0; l < d.L; ++l) std::memcpy(et + (CEM_ET_ROWS + 2 * l) * CEM_U, nat + no.b[l], d.U * 4);
        }
        HIPCHK(hipMemcpyAsync(h->ws + h->lay.etab, h->h_etab.data(), h->h_etab.size() * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        h->have_weights = true;
        return CEM_OK;
    }
    std::vector<float> packed((size_t)d.member_stride_f4 * 4 * d.E);
    std::vector<float> bh((size_t)d.E * d.L * CEM_U, 0.f), bmu((size_t)d.E * CEM_U, 0.f), bvar((size_t)d.E * CEM_U, 0.f);
    const NatOff no = nat_offsets(d);
    for (int m = 0; m < d.E; ++m) {
        const float *nat = blob + (size_t)m * d.nat_member_floats;
        if (d.chunked()) pack_member_chunked(d, nat, reinterpret_cast<uint16_t *>(packed.data() + (size_t)m * d.member_stride_f4 * 4));
        else pack_member(d, nat, packed.data() + (size_t)m * d.member_stride_f4 * 4);
        for (int l = 0; l < d.L; ++l) std::memcpy(&bh[((size_t)m * d.L + l) * CEM_U], nat + no.b[l], d.U * 4);
        std::memcpy(&bmu[(size_t)m * CEM_U], nat + no.bmu, d.O * 4);
        std::memcpy(&bvar[(size_t)m * CEM_U], nat + no.bvar, d.O * 4);
    }
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.wpack, packed.data(), packed.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.bias_h, bh.data(), bh.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.bias_mu, bmu.data(), bmu.size() * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.bias_var, bvar.data(), bvar.size() * 4, hipMemcpyHostToDevice, h->stream));
    {   // the same biases as rows of the hot kernel's per-member table
        const size_t et_rows = etab_rows(d);
        for (int m = 0; m < d.E; ++m) {
            float *et = &h->h_etab[(size_t)m * et_rows * CEM_U];
            std::memcpy(et + CEM_ET_BMU * CEM_U, &bmu[(size_t)m * CEM_U], CEM_U * 4);
            std::memcpy(et + CEM_ET_BVAR * CEM_U, &bvar[(size_t)m * CEM_U], CEM_U * 4);
            for (int l = 0; l < d.L; ++l) std::memcpy(et + (CEM_ET_ROWS + l) * CEM_U, &bh[((size_t)m * d.L + l) * CEM_U], CEM_U * 4);
        }
        HIPCHK(hipMemcpyAsync(h->ws + h->lay.etab, h->h_etab.data(), h->h_etab.size() * 4, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    h->have_weights = true;
    return CEM_OK;
}

int cem_planner_set_weights_dev(cem_planner_t *h, const float *blob_dev, size_t n_floats)
{
    if (!h || !blob_dev) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    if (n_floats != d.nat_member_floats * d.E) return CEM_ERR_INVALID_ARG;
    cem_pack_trained_t p{};
    p.blob = blob_dev; p.desc = h->pack_desc; p.nat = (uint32_t)d.nat_member_floats; p.n_desc = h->n_pack_desc; p.E = (uint32_t)d.E;
    if (d.wide) {
        p.blob_copy = (float *)(h->ws + h->lay.wpack); p.dst = h->ws + h->lay.wpack + align256(n_floats * 4);
        p.member_bytes = wide_image_floats(d) * 4; p.n_slack = 0;
    } else {
        p.dst = h->ws + h->lay.wpack; p.member_bytes = (unsigned long long)d.member_stride_f4 * 16; p.n_slack = 4;     // the +256 float4 of slack
    }
    const unsigned wgs = (p.n_desc + p.n_slack + CEM_PACK_WAVES - 1) / CEM_PACK_WAVES;
    const dim3 grid(wgs * (unsigned)d.E), block(64 * CEM_PACK_WAVES);
    if (d.wide) hipLaunchKernelGGL(cem_pack_wide_kernel, grid, block, 0, h->stream, p);
    else if (d.split()) hipLaunchKernelGGL(cem_pack_split_kernel, grid, block, 0, h->stream, p);
    else if (d.bf16()) launch_pack_bf16(p, grid.x, h->stream);
    else hipLaunchKernelGGL(cem_pack_fp32_kernel, grid, block, 0, h->stream, p);
    cem_pack_trained_bias_t b{};
    b.blob = blob_dev; b.bias_h = (float *)(h->ws + h->lay.bias_h); b.bias_mu = (float *)(h->ws + h->lay.bias_mu);
    b.bias_var = (float *)(h->ws + h->lay.bias_var); b.etab = (float *)(h->ws + h->lay.etab);
    b.nat = p.nat; b.Din = (uint32_t)d.Din; b.U = (uint32_t)d.U; b.L = (uint32_t)d.L; b.O = (uint32_t)d.O; b.E = p.E; b.wide = d.wide ? 1u : 0u;
    const size_t quads = (size_t)d.E * (2 + (d.wide ? 2 : 1) * (size_t)d.L) * (CEM_U / 4);
    hipLaunchKernelGGL(cem_pack_bias_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, h->stream, b);
    HIPCHK(hipGetLastError());
    h->have_weights = true;                              // (no synchronise: plans queued behind this on the handle's stream see the new images)
    return CEM_OK;
}

int cem_planner_set_normaliser(cem_planner_t *h, const float *imin, const float *imax)
{
    if (!h || !imin || !imax) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    std::vector<float> mn(CEM_U, 0.f), dl(CEM_U, 1.f);
    if (h->cfg.scale_features) {                      // transition_model.py:79-87
        for (int f = 0; f < d.Din; ++f) {
            float delta = imax[f] - imin[f];
            if (delta < 1e-5f) delta = 1.01f;
            mn[f] = imin[f]; dl[f] = 1.0f / delta;      // the kernel multiplies by 1/delta (<= 1.5 ulp from the reference's division)
        }
    }
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.nmin, mn.data(), CEM_U * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.ndelta, dl.data(), CEM_U * 4, hipMemcpyHostToDevice, h->stream));
    {
        const size_t et_rows = etab_rows(d);
        for (int m = 0; m < d.E; ++m) {
            float *et = &h->h_etab[(size_t)m * et_rows * CEM_U];
            std::memcpy(et + CEM_ET_NMIN * CEM_U, mn.data(), CEM_U * 4);
            std::memcpy(et + CEM_ET_RDELTA * CEM_U, dl.data(), CEM_U * 4);
        }
        // only the two rows this call owns, in every member's table: the bias rows of the host copy are those of the last HOST
        // set_weights, and after cem_planner_set_weights_dev the device holds newer ones
        for (int row : {CEM_ET_NMIN, CEM_ET_RDELTA})
            HIPCHK(hipMemcpy2DAsync(h->ws + h->lay.etab + (size_t)row * CEM_U * 4, et_rows * CEM_U * 4, h->h_etab.data() + (size_t)row * CEM_U,
                                    et_rows * CEM_U * 4, CEM_U * 4, (size_t)d.E, hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------------------
namespace {

template <int RC, int NFW, int MODE>
hipError_t launch_rollout_t(const RolloutParams &p, int n_tiles, hipStream_t st)
{
    const size_t lds = CEM_ROLLOUT_LDS_BYTES(RC);
    hipLaunchKernelGGL((cem_rollout_kernel<RC, NFW, MODE>), dim3(n_tiles), dim3(256), lds, st, p);
    return hipGetLastError();
}

template <int RC, int NFW>
hipError_t launch_rollout_seg_t(const RolloutParams &p, int grid, hipStream_t st)
{
    const size_t lds = CEM_ROLLOUT_LDS_BYTES(RC);
    hipLaunchKernelGGL((cem_rollout_seg_kernel<RC, NFW>), dim3(grid), dim3(256), lds, st, p);
    return hipGetLastError();
}

hipError_t launch_rollout_seg(int rc, int nfw, const RolloutParams &p, int grid, hipStream_t st)
{
    return with_tile_shape(rc, nfw, hipErrorInvalidValue, [&](auto R, auto F) { return launch_rollout_seg_t<R(), F()>(p, grid, st); });
}

template <int MODE>
hipError_t launch_rollout(int rc, int nfw, const RolloutParams &p, int n_tiles, hipStream_t st)
{
    return with_tile_shape(rc, nfw, hipErrorInvalidValue, [&](auto R, auto F) { return launch_rollout_t<R(), F(), MODE>(p, n_tiles, st); });
}

// the chunked rollouts (cem_rollout_chunked.h), whole-horizon tiles; mode 1 = caller-supplied noise tensors.  The split kernels are
// this unit's, the bf16 kernels cem_rollout_bf16.hip's: the same dispatch, expanded where the kernels are.
CEM_CHUNKED_LAUNCHER(launch_rollout_split, cem_rollout_split_kernel, 3)
hipError_t launch_rollout_chunked(const Dims &d, int rc, int mode, const RolloutParams &p, int n_tiles, hipStream_t st)
{
    return (d.split() ? launch_rollout_split : launch_rollout_bf16)(rc, d.NFW, mode, p, n_tiles, st);
}

// mode 0: planning; mode 1: caller-supplied action / noise tensors, trajectory and head-moment outputs
hipError_t launch_rollout_wide(const cem_planner *h, const RolloutParams &rp, int n_tiles, int mode)
{
    WideParams wp; wp.r = rp;
    wp.U = h->d.U; wp.act = h->cfg.activation;
    wp.wimg = (const f4 *)(h->ws + h->lay.wpack + align256((size_t)h->d.E * h->d.nat_member_floats * 4)); wp.img_f4 = (uint32_t)(wide_image_floats(h->d) / 4);
    if (mode == 0) hipLaunchKernelGGL(cem_rollout_wide_kernel<0>, dim3(n_tiles), dim3(256), CEM_WIDE_SMEM, h->stream, wp);
    else hipLaunchKernelGGL(cem_rollout_wide_kernel<1>, dim3(n_tiles), dim3(256), CEM_WIDE_SMEM, h->stream, wp);
    return hipGetLastError();
}

// dv: the shape of a scheduled iteration (cem_population.h), else the handle's own
void fill_rollout_common(const cem_planner *h, RolloutParams &p, const Dims *dv = nullptr)
{
    const Dims &d = dv ? *dv : h->d; const Layout &l = h->lay; char *ws = h->ws;
    std::memset(&p, 0, sizeof(p));
    p.wpack = (const f4 *)(ws + l.wpack); p.bias_h = (const float *)(ws + l.bias_h);
    p.bias_mu = (const float *)(ws + l.bias_mu); p.bias_var = (const float *)(ws + l.bias_var);
    p.nmin = (const float *)(ws + l.nmin); p.nrdelta = (const float *)(ws + l.ndelta);
    p.omask = (const float *)(ws + l.omask); p.kind_sel = (const float *)(ws + l.kind_sel);
    p.etab = (const float *)(ws + l.etab);
    p.act_pad = (const f4 *)(ws + l.act_pad); p.act_pad_bytes = (uint32_t)((size_t)d.N * d.H * d.act_nq * 16); p.act_q0 = d.act_q0; p.act_nq = d.act_nq;
    p.ctrl = (const CtrlBlock *)(ws + l.ctrl);
    p.member_stride_f4 = d.member_stride_f4;
    for (int w = 0; w < 4; ++w) { p.wave_off_f4[w] = d.wave_off_f4[w]; p.wave_groups[w] = (uint32_t)d.wave_groups[w]; }
    p.O = d.O; p.A = d.A; p.L = d.L; p.KB_in = d.KB_in; p.KB_obs = d.KB_obs;
    p.sampling = h->cfg.sampling_propagation; p.sc = h->sc_roll;
}

hipEvent_t get_event(cem_planner *h, size_t i)
{
    while (h->ev.size() <= i) { hipEvent_t e; hipEventCreate(&e); h->ev.push_back(e); }
    return h->ev[i];
}

// Times what is launched within its scope as `kind` (0 rollout / 1 select / 2 reduce / 3 sampler launch) when timing is on: the start
// event and the ev_kind entry now, the stop event at stop() or at the end of the scope.  Nothing when timing is off.
struct TimedLaunch {
    cem_planner *h; size_t e0;
    TimedLaunch(cem_planner *h_, int kind) : h(h_->timing ? h_ : nullptr), e0(0)
    {
        if (!h) return;
        e0 = h->ev_kind.size() * 2; h->ev_kind.push_back({(int)e0, kind}); hipEventRecord(get_event(h, e0), h->stream);
    }
    void stop() { if (h) hipEventRecord(get_event(h, e0 + 1), h->stream); h = nullptr; }
    ~TimedLaunch() { stop(); }
};

void warm_handed_over(cem_planner *h);

int enqueue_begin(cem_planner *h)
{
    const Dims &d = h->d; const Layout &l = h->lay;
    InitParams ip{}; ip.ctrl = (CtrlBlock *)(h->ws + l.ctrl); ip.musig = (float *)(h->ws + l.musig); ip.HA = d.H * d.A; ip.A = d.A;
    ip.host_ctrl = h->d_h_ctrl;                          // the block stage_ctrl filled, read from pinned host memory by the kernel itself
    for (int a = 0; a < d.A; ++a) { ip.mu0[a] = h->cfg.act_mu0[a]; ip.sigma0[a] = h->cfg.act_sigma0[a]; }
    if (!h->pop.empty()) {                               // a schedule: the most FIFO entries any of its iterations uses (cem_population.h)
        if (h->pop_n_ready > 0) { ip.seg_queue = (uint32_t *)(h->ws + l.seg_queue); ip.seg_flags = h->pop_seg_flags; ip.n_ready = h->pop_n_ready; }
    } else
    if (h->n_seg > 1) { ip.seg_queue = (uint32_t *)(h->ws + l.seg_queue); ip.seg_flags = (uint32_t *)(h->ws + l.seg_flags); ip.n_ready = (h->n_tiles - h->n_pinned) * (h->n_seg - 1); }
    ip.n_prob = h->batch;                                // a batch handle: every problem's block and mu / sigma (the done ones included)
    ip.warm = h->d_h_warm; ip.carry = (float *)(h->ws + l.carry); ip.expl = (const float *)(h->ws + l.expl);
    const int n = warm_slots(h) * std::max<int>(ip.HA, (int)(sizeof(CtrlBlock) / 4));
    hipLaunchKernelGGL(cem_init_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, ip);
    HIPCHK(hipGetLastError());
    // time-correlated action noise: the plan's whole eps_act tensor, from the key the kernel above has just put into the workspace (one
    // launch and one graph node per plan); a caller's own eps_act is taken as given
    if (h->opt.noise_kind == CEM_NOISE_MIXED && !h->eps_act) {
        MixParams mp{}; mp.mix_t = h->noise_dev; mp.eps = h->noise_eps; mp.ctrl = (const CtrlBlock *)(h->ws + l.ctrl);
        mp.I = d.I; mp.N = d.N; mp.H = d.H; mp.A = d.A;
        HIPCHK(launch_mix_action_noise(mp, warm_slots(h), h->stream));
    }
    {   // launched for real (not recorded into a graph): the pending carries are on their way to Layout::carry (stage_warm's invariant)
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(h->stream, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
        if (cs == hipStreamCaptureStatusNone) warm_handed_over(h);
    }
    return CEM_OK;
}

// cem_planner_constraint_costs reads the PLAN's C array from here on (not cem_compute_objective's own): said by every constrained reduce
// that is enqueued and by run_plan, since a replayed graph passes through no enqueue function
void note_plan_cstat(cem_planner *h)
{
    const int nb = warm_slots(h);
    h->last_cstat = h->budget_dev + nb; h->last_cstat_n = h->d.Nloc; h->last_cstat_problems = nb;
}

// The score stage (cem_score.h) of the handle's objective.  The caller says what differs between a plan and the standalone op — the
// buffers, the shape, whether a finished plan skips it and whether it clears the select's words; the handle says the rest.
ReduceParams fill_score(const cem_planner *h, const float *ret, const uint8_t *costs, float *scores, float *cstat, int Nloc, int H, int check_done, bool clear_select)
{
    ReduceParams p{}; p.ret = ret; p.costs = costs; p.scores = scores; p.ctrl = (const CtrlBlock *)(h->ws + h->lay.ctrl);
    p.Nloc = Nloc; p.P = h->d.P; p.H = H; p.variant = h->cfg.variant; p.check_done = check_done;
    p.alpha = h->alpha; p.beta = h->beta; p.thr = h->cfg.posterior_mean_threashold;
    if (clear_select) { p.zero = (uint32_t *)(h->ws + h->lay.ms_hist); p.zero_n = CEM_MS_CLEAR_BYTES / 4; }
    // one m serves both: the setters refuse a lower tail on a budget handle and the reverse, and a COST handle refuses both, so at most one of
    // cost_m / tail_m is set; a kernel that reads neither m nor budget ignores them
    p.m = h->opt.cost_m ? h->opt.cost_m : h->opt.tail_m; p.cstat = cstat; p.budget = h->budget_dev;
    return p;
}

// the one place a score kernel is chosen: grid.x = blocks of 64 candidates, grid.y = problems of a batched plan
hipError_t launch_score(const cem_planner *h, const ReduceParams &p, int n_problems)
{
    const dim3 grid((p.Nloc + 63) / 64, n_problems), block(CEM_SCORE_THREADS);
    if (h->cfg.variant == CEM_VARIANT_COST) hipLaunchKernelGGL(cem_constraint_reduce_kernel, grid, block, 0, h->stream, p);
    else if (h->opt.cost_m) hipLaunchKernelGGL(cem_constrained_budget_kernel, grid, block, CEM_BUDGET_LDS_BYTES(p.P, p.m), h->stream, p);
    else if (h->opt.tail_m) hipLaunchKernelGGL(cem_constraint_tail_kernel, grid, block, CEM_TAIL_LDS_BYTES(p.P), h->stream, p);
    else hipLaunchKernelGGL(cem_reduce_kernel, grid, block, 0, h->stream, p);
    return hipGetLastError();
}

// the parameter block of the two carry-over kernels in iteration `it`
EliteCarryParams fill_elite(const cem_planner *h, int it)
{
    const IterView v = iter_view(h, it);
    const Dims &d = *v.d; const Layout &l = h->lay; char *ws = h->ws;
    EliteCarryParams ep{}; ep.scores = (const float *)(ws + l.scores_global); ep.actions = (float *)(ws + l.actions); ep.act_pad = (float *)(ws + l.act_pad);
    ep.ctrl = (const CtrlBlock *)(ws + l.ctrl); ep.elite_idx = (const int32_t *)(ws + l.elite); ep.store = elite_store(h); ep.count = elite_counts(h);
    ep.N = d.N; ep.k = d.k; ep.m = h->opt.elite.n_keep; ep.H = d.H; ep.A = d.A; ep.it = it; ep.shift = h->opt.elite.across_plans ? h->opt.elite.shift : 0;
    ep.pad_shift = d.O - 4 * d.act_q0; ep.pad_floats = 4 * d.act_nq;
    return ep;
}

// One iteration up to the scores, as its recipe says: the rollout launch (its tiles sample their own action sequences first:
// cem_tile_sample_actions), then the particle mean / Beta filter — unless the reduce is folded: a single-rank `whole_plan` on the CemMpc
// objective lets the select kernel form the particle mean while it stages its keys (same sum, same order, one launch and one graph
// node fewer per iteration).  The stepwise form always leaves the scores in scores_local (the caller may exchange them).
int enqueue_rollout(cem_planner *h, int it, bool whole_plan)
{
    const LaunchRecipe rc = recipe_of(h, it, h->eps_act || h->eps_model);
    // v: what this iteration launches — the handle's plan, or the scheduled iteration's (cem_population.h); d: its shape.  The caller's
    // noise tensors keep the slabs of the handle's own n_samples (h->d), of which a narrower iteration reads the leading part
    const IterView v = iter_view(h, it);
    const Dims &d = *v.d; const Layout &l = h->lay; char *ws = h->ws;
    const bool queued = v.n_seg > 1 && !h->eps_model && !rc.task;   // explicit eps_model tensors and the task scorer take the general (MODE 1) kernel
    if (rc.task && !h->task_dev) return CEM_ERR_UNSUPPORTED;        // (the setter made the allocation before it committed)
    RolloutParams rp; fill_rollout_common(h, rp, v.d);
    rp.tiles = v.tiles; rp.s0 = nullptr; rp.actions = (const float *)(ws + l.actions);
    rp.eps_model = h->eps_model ? h->eps_model + (size_t)it * d.H * h->d.Btot * d.O : nullptr;
    // CEM_VARIANT_COST: the safe variant's launch (its cost bytes, un-masked by sc_roll's threshold); the returns it also writes mean nothing
    const bool cost_obj = h->cfg.variant == CEM_VARIANT_COST;
    rp.ret = (float *)(ws + l.returns); rp.costs = h->cfg.variant != CEM_VARIANT_CEM ? (uint8_t *)(ws + l.costs) : nullptr;
    rp.H = d.H; rp.Bloc = d.Bloc; rp.Btot = d.Btot; rp.it = it; rp.variant = cost_obj ? (int)CEM_VARIANT_SAFE : h->cfg.variant; rp.check_done = 1;
    rp.stamps = (long long *)(ws + l.stamps);
    // the sampler's inputs and outputs (cem_mpc.py:44-48)
    // (the handle's own mixed tensor stands in wherever the caller passed none)
    const float *eps_act = h->eps_act ? h->eps_act : (h->opt.noise_kind == CEM_NOISE_MIXED ? h->noise_eps : nullptr);
    rp.musig = (const float *)(ws + l.musig); rp.eps_act = eps_act ? eps_act + (size_t)it * h->d.N * d.H * d.A : nullptr;
    rp.act_bounds = (const float *)(ws + l.act_bounds); rp.actions_w = (float *)(ws + l.actions); rp.act_pad_w = (float *)(ws + l.act_pad);
    rp.pad_shift = d.O - 4 * d.act_q0; rp.pad_floats = 4 * d.act_nq; rp.N = d.N; rp.Nloc = d.Nloc; rp.n_off = d.n_off; rp.n_tiles = v.n_tiles;
    // a batch handle: ONE launch per stage for all its problems, problem b on tiles [b n_tiles, (b + 1) n_tiles) and its own slices
    const int nb = warm_slots(h);
    rp.tiles_per_problem = h->batch ? v.n_tiles : 0;
    rp.eps_act_pstride = (long long)d.I * h->d.N * d.H * d.A; rp.eps_model_pstride = (long long)d.I * d.H * h->d.Btot * d.O;
    if (rc.sampler_launch) {                                  // all N candidates once, in front of the rollout launch (which then samples nothing)
        const int total = d.N * d.H * ((d.A + 3) / 4);
        TimedLaunch timed(h, 3);
        hipLaunchKernelGGL(cem_sample_kernel, dim3(std::min((total + 255) / 256, 2048), nb), dim3(256), 0, h->stream, rp);
        HIPCHK(hipGetLastError());
        rp.musig = nullptr;
        // elite carry-over: rows 0 .. count - 1 of the sample become the kept elites (cem_elite_carry.h).  Iteration 0 has nothing of this
        // plan to take; across_plans lets the device-side count decide there, so that one captured graph serves the first plan and later ones
        if (rc.inject_elites && (it > 0 || h->opt.elite.across_plans)) {
            EliteCarryParams ep = fill_elite(h, it);
            HIPCHK(launch_elite_inject(ep, nb, h->stream));
        }
        // the mean candidate: the iteration's last row becomes the clipped mu it was sampled from (cem_population.h)
        if (rc.inject_mean) {
            MeanCandidateParams mc{}; mc.musig = (const float *)(ws + l.musig); mc.act_bounds = rp.act_bounds; mc.ctrl = rp.ctrl;
            mc.actions = rp.actions_w; mc.act_pad = rp.act_pad_w; mc.N = d.N; mc.row = d.N - 1; mc.H = d.H; mc.A = d.A;
            mc.pad_shift = rp.pad_shift; mc.pad_floats = rp.pad_floats;
            HIPCHK(launch_mean_candidate(mc, nb, h->stream));
        }
    }
    // the task scorer: the family's MODE 1 instantiation (cem_unfold_sequences'), its raw states into the handle's buffer; Philox model
    // noise unless the caller brought a tensor
    const bool mode1 = rp.eps_model || rc.task;
    if (rc.task) rp.traj = task_traj(h);
    TimedLaunch timed(h, 0);
    // a segmented launch: its work queue into rp, and its grid — one workgroup per pinned tile, then one per (floating tile, segment) item
    const auto queue_grid = [&] {
        rp.seg_queue = (uint32_t *)(ws + l.seg_queue); rp.seg_flags = v.seg_flags; rp.seg_state = v.seg_state;
        rp.seg_len = v.seg_len; rp.n_seg = v.n_seg; rp.n_pinned = v.n_pinned;
        return v.n_pinned + v.n_seg * (v.n_tiles - v.n_pinned);
    };
    if (rc.lean_form) {                                          // (the same tiles, segments and work queue as the generic launches below)
        const int grid = queued ? queue_grid() : v.n_tiles;
        if (rc.lean_form == 2 && (rp.variant == 1) == (rp.costs != nullptr)) HIPCHK(launch_rollout_lean_straight(rp, grid, h->stream, queued));
        else HIPCHK(launch_rollout_lean(rp, grid, h->stream, queued));
    }
    else if (d.wide) HIPCHK(launch_rollout_wide(h, rp, v.n_tiles, mode1 ? 1 : 0));
    else if (d.chunked()) HIPCHK(launch_rollout_chunked(d, v.rc, mode1 ? 1 : 0, rp, v.n_tiles, h->stream));
    else if (mode1) HIPCHK(launch_rollout<1>(v.rc, d.NFW, rp, nb * v.n_tiles, h->stream));
    else if (queued) HIPCHK(launch_rollout_seg(v.rc, d.NFW, rp, queue_grid(), h->stream));
    else HIPCHK(launch_rollout<0>(v.rc, d.NFW, rp, nb * v.n_tiles, h->stream));
    timed.stop();
    // the task's returns and cost bytes over the Safety-Gym ones the rollout has just written, in stream order (cem_task_tile.h);
    // timed with the reduce
    if (rc.task) {
        TaskParams io{};
        io.traj = rp.traj; io.actions = rp.actions; io.ctrl = rp.ctrl; io.ret = rp.ret; io.costs = rp.costs;
        io.rows = d.Bloc; io.N = d.N; io.H = d.H; io.check_done = 1;
        TimedLaunch timed_task(h, 2);
        { const int st = task_launch(h, io, CEM_ERR_UNSUPPORTED); if (st) return st; }
    }
    if (whole_plan && rc.fold_reduce) return CEM_OK;

    // the score kernel of the handle's objective, timed as the one reduce launch; it clears the words of this iteration's multi-workgroup select
    const ReduceParams sp = fill_score(h, rp.ret, rp.costs, (float *)(ws + l.scores_local), h->opt.cost_m ? h->budget_dev + nb : nullptr, d.Nloc, d.H, 1, true);
    h->sel_zeroed = true;
    if (h->opt.cost_m) note_plan_cstat(h);
    TimedLaunch timed_reduce(h, 2);
    HIPCHK(launch_score(h, sp, nb));
    return CEM_OK;
}

// whole_plan: the select forms the particle mean where the recipe folds it, and writes the plan's result itself where it can (eps_out is
// known before the loop) — returns through *folded whether it did (only the one-workgroup kernel does), so the caller knows whether a
// final kernel is still needed
int enqueue_select(cem_planner *h, int it, bool whole_plan, bool have_eps_out = false, bool *folded = nullptr)
{
    if (folded) *folded = false;
    const LaunchRecipe rc = recipe_of(h, it, h->eps_act || h->eps_model);
    const bool fold_reduce = whole_plan && rc.fold_reduce, fold_final = whole_plan;
    const Dims &d = *iter_view(h, it).d; const Layout &l = h->lay; char *ws = h->ws;    // (a scheduled iteration ranks its own n[it] candidates)
    SelectParams p{}; p.scores = (const float *)(ws + l.scores_global); p.actions = (const float *)(ws + l.actions);
    p.musig = (float *)(ws + l.musig); p.ctrl = (CtrlBlock *)(ws + l.ctrl); p.elite_idx = (int32_t *)(ws + l.elite);
    p.N = d.N; p.k = d.k; p.HA = d.H * d.A; p.A = d.A; p.check_done = 1;
    p.smoothing = h->cfg.smoothing; p.one_minus_smoothing = h->cfg.one_minus_smoothing; p.threshold = h->cfg.stddev_threshold;
    p.stamps = (long long *)(ws + l.stamps) + 64;          // past tile 0's rollout stamps; written by -DCEM_STAMPS builds only
    if (fold_reduce) { p.ret = (const float *)(ws + l.returns); p.P = d.P; p.scores_w = (float *)(ws + l.scores_local); }   // (LaunchRecipe::fold_reduce: world 1, so local == global)
    size_t lds = (size_t)((d.k + 3) & ~3) * 4 + (size_t)2 * d.H * d.A * 4;
    // Large populations (the replicated select of a many-GPU plan) go through multi-workgroup kernels (cem_mpc.h select_mode):
    // the fused form (one launch, grid barriers) whenever all its ceil(N / 4096) workgroups are resident at once, the eight-launch
    // chain beyond that (more workgroups than CUs), the one-workgroup kernel for populations it still serves faster.  Measured
    // (profiles/r03_select_forms.txt, us per select at N = 8000 / 16000 / 40000 / 65536): one workgroup 27 / 44 / 111 / 171, chain
    // 68 / 71 / 78 / 83, fused 60 / 61 / 69 / 76 — a grid barrier is an atomic and a poll at the device coherence point (~4 us with
    // the XCDs' L2s not coherent with each other), hardly cheaper than a kernel boundary inside a graph: the cross-over with the
    // one-workgroup kernel stays near 24 000 keys.
    // The fused form's grid barriers need all G workgroups resident at once: G is held against what the RUNTIME says the device keeps
    // resident of this kernel (asked once at create: workgroups per CU x CUs), not against the CU count alone.  What it cannot see is
    // other work on the device — another stream, handle or process, a CU-masked queue: the form assumes a GPU that is otherwise idle
    // for the few microseconds of the launch; under contention a barrier times out (bounded polls), cem_msel_solo_kernel redoes that
    // iteration's select in stream order (the plan stays valid, with select_mode 2's bits) and the handle stops fusing: read_results,
    // select_mode_now.  select_mode 2 has no such assumption.
    const int G = (d.N + CEM_MS_KEYS - 1) / CEM_MS_KEYS;
    const int mode = rc.select_mode; const bool cache = rc.select_cache;
    if (mode == 0) return CEM_ERR_UNSUPPORTED;          // (an explicit select_mode 1 on a device that grants less dynamic LDS than validate() assumed)
    // The score-weighted refit (cem_refit_weighted.h): the one-workgroup select as it is, blending into a scratch slice, never stopping and
    // never handing over the result; cem_constraint_refit_kernel behind it refits the plan's mu / sigma and decides the early stop.
    const bool weighted = rc.weighted;
    // (admit() let these onto one-workgroup handles only, and their setters made the allocations before they committed)
    if (rc.one_workgroup_only && (mode != 1 || (weighted && !h->refit_dev) || (rc.keep_elites && !h->elite_dev) || (rc.track && !h->readout_dev))) return CEM_ERR_UNSUPPORTED;
    if (weighted) { p.musig = h->refit_dev; p.threshold = -std::numeric_limits<float>::infinity(); }
    TimedLaunch timed(h, 1);
    if (mode >= 2) {
        MSelParams m{}; m.scores = p.scores; m.actions = p.actions; m.musig = p.musig; m.ctrl = p.ctrl; m.elite_idx = p.elite_idx;
        m.hist = (uint32_t *)(ws + l.ms_hist); m.sel = (uint32_t *)(ws + l.ms_sel); m.wg_counts = (uint32_t *)(ws + l.ms_counts);
        m.bar = m.sel + 8;
        m.best_sc = (float *)(ws + l.ms_best_sc); m.best_ix = (int32_t *)(ws + l.ms_best_ix);
        m.part = (float *)(ws + l.ms_part); m.colmean = (float *)(ws + l.ms_colmean);
        m.N = d.N; m.k = d.k; m.HA = p.HA; m.A = d.A; m.check_done = 1; m.smoothing = p.smoothing; m.one_minus_smoothing = p.one_minus_smoothing; m.threshold = p.threshold;
        m.G = G; m.G2 = (d.k + CEM_MS_EPG - 1) / CEM_MS_EPG;
        // the histograms and the barrier counter (adjacent in the workspace) start at zero; within a plan the reduce kernel of the
        // same iteration has already cleared them (ReduceParams::zero), this memset covers a select called on its own
        if (!h->sel_zeroed) HIPCHK(hipMemsetAsync(m.hist, 0, CEM_MS_CLEAR_BYTES, h->stream));
        h->sel_zeroed = false;
        if (mode == 3) {
            hipLaunchKernelGGL(cem_msel_fused_kernel, dim3(m.G), dim3(1024), 0, h->stream, m);
            // returns at once unless a grid barrier of the launch above expired; then it redoes this iteration's select alone (cem_device.h)
            hipLaunchKernelGGL(cem_msel_solo_kernel, dim3(1), dim3(1024), 0, h->stream, m);
        } else {
            hipLaunchKernelGGL(cem_msel_hist_kernel<0>, dim3(m.G), dim3(1024), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_hist_kernel<1>, dim3(m.G), dim3(1024), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_hist_kernel<2>, dim3(m.G), dim3(1024), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_count_kernel, dim3(m.G), dim3(1024), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_compact_kernel, dim3(m.G), dim3(1024), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_moments_kernel<0>, dim3(m.G2), dim3(256), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_moments_kernel<1>, dim3(m.G2), dim3(256), 0, h->stream, m);
            hipLaunchKernelGGL(cem_msel_final_kernel, dim3(1), dim3(256), 0, h->stream, m);
        }
    } else {
        if (fold_final && !h->batch && !weighted) {     // (a batch handle: the final kernel writes every problem's result, then the completion markers)
            p.is_last = it == d.I - 1;
            p.result = h->d_h_result; p.result_dev = (uint32_t *)(ws + l.result); p.eps_out = have_eps_out ? (const float *)(ws + l.eps_out) : nullptr; p.noise_stddev = h->cfg.noise_stddev;
            if (folded) *folded = true;
        }
        if (cache) lds += (size_t)CEM_SEL_KWORDS(d.N) * 4;
        // (SafeCemMpc's scores have a crowd near -100, the cost objective's crowd into a few multiples of 1 / P: the instantiation that
        // counts and ranks wave by wave; same results either way)
        // one workgroup per problem (batch handles: blockIdx.x is the problem)
        const dim3 grid(warm_slots(h));
        if (rc.select_form == 1) HIPCHK(launch_select_ranked(p, warm_slots(h), lds, h->stream));     // (the same p, grid and LDS bytes)
        else if (cache && h->cfg.variant != CEM_VARIANT_CEM) hipLaunchKernelGGL((cem_select_kernel<true, true>), grid, dim3(1024), lds, h->stream, p);
        else if (cache) hipLaunchKernelGGL((cem_select_kernel<true, false>), grid, dim3(1024), lds, h->stream, p);
        else hipLaunchKernelGGL((cem_select_kernel<false, false>), grid, dim3(1024), lds, h->stream, p);
        if (weighted) {
            HIPCHK(hipGetLastError());
            RefitWeightedParams rw{}; rw.scores = p.scores; rw.actions = p.actions; rw.musig = (float *)(ws + l.musig); rw.ctrl = p.ctrl; rw.elite_idx = p.elite_idx;
            rw.stat = h->refit_dev + (size_t)warm_slots(h) * 2 * p.HA;
            rw.N = d.N; rw.k = d.k; rw.HA = p.HA; rw.I = d.I; rw.beta = h->refit_beta;
            rw.smoothing = p.smoothing; rw.one_minus_smoothing = p.one_minus_smoothing; rw.threshold = h->cfg.stddev_threshold;
            HIPCHK(launch_refit_weighted(rw, warm_slots(h), h->stream));
            h->refit_ran = true;
        }
        // elite carry-over: the best n_keep of the elites just chosen, for the next iteration's (the next plan's) inject
        if (rc.keep_elites) {
            HIPCHK(hipGetLastError());
            const EliteCarryParams ep = fill_elite(h, it);
            HIPCHK(launch_elite_keep(ep, warm_slots(h), h->stream));
        }
        // the plan read-out: the best-so-far candidate's sequence, returns and cost counts leave the workspace before the next rollout
        // overwrites them (cem_plan_readout.h).  Last: every launch above stays where it was; device-side state only (the control
        // block in the workspace, never the pinned staging the next plan call writes while this launch may still be running)
        if (rc.track) {
            HIPCHK(hipGetLastError());
            PlanTrackParams tp{}; tp.scores = p.scores; tp.actions = p.actions; tp.ret = (const float *)(ws + l.returns);
            tp.costs = h->cfg.variant != CEM_VARIANT_CEM ? (const uint8_t *)(ws + l.costs) : nullptr;
            tp.ctrl = p.ctrl; tp.elite_idx = p.elite_idx; tp.block = h->readout_dev;
            tp.N = d.N; tp.k = d.k; tp.H = d.H; tp.A = d.A; tp.P = d.P; tp.it = it; tp.stride = (int32_t)CEM_READOUT_WORDS(h->d.H, h->d.A, h->d.P);
            HIPCHK(launch_plan_track(tp, warm_slots(h), h->stream));
        }
    }
    HIPCHK(hipGetLastError());
    return CEM_OK;
}

// the one exchange step of an iteration: every rank's N/world local scores -> all N scores on every rank
int enqueue_exchange(cem_planner *h)
{
    if (!h->comm) return CEM_OK;
    Rccl *r = rccl(); if (!r) return CEM_ERR_COMM;
    const Dims &d = h->d; const Layout &l = h->lay;
    // world 1: scores_global aliases scores_local and the all-gather is the in-place form (sendbuff == recvbuff + rank * count)
    NCCLCHK(r->AllGather(h->ws + l.scores_local, h->ws + l.scores_global, (size_t)d.Nloc, kNcclFloat32, h->comm, h->stream));
    return CEM_OK;
}

int enqueue_end(cem_planner *h, bool have_eps_out)
{
    const Dims &d = h->d; const Layout &l = h->lay; char *ws = h->ws;
    if (h->batch) {
        FinalBatchParams fb{}; fb.ctrl = (const CtrlBlock *)(ws + l.ctrl); fb.eps_out = have_eps_out ? (const float *)(ws + l.eps_out) : nullptr;
        fb.result = h->d_h_result; fb.result_dev = (uint32_t *)(ws + l.result); fb.A = d.A; fb.n_prob = h->batch; fb.noise_stddev = h->cfg.noise_stddev;
        hipLaunchKernelGGL(cem_final_batch_kernel, dim3(1), dim3(256), 0, h->stream, fb);
        HIPCHK(hipGetLastError());
        return CEM_OK;
    }
    FinalParams fp{}; fp.ctrl = (const CtrlBlock *)(ws + l.ctrl); fp.eps_out = have_eps_out ? (const float *)(ws + l.eps_out) : nullptr;
    fp.result = h->d_h_result; fp.result_dev = (uint32_t *)(ws + l.result); fp.A = d.A; fp.noise_stddev = h->cfg.noise_stddev;       // pinned host memory: no copy node behind the kernel
    hipLaunchKernelGGL(cem_final_kernel, dim3(1), dim3(64), 0, h->stream, fp);
    HIPCHK(hipGetLastError());
    return CEM_OK;
}

void collect_timing(cem_planner *h)
{
    h->roll_ms = 0.f; h->sel_ms = 0.f; h->red_ms = 0.f; h->samp_ms = 0.f; h->roll_n = 0;
    for (auto &ek : h->ev_kind) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev[ek.first], h->ev[ek.first + 1]) == hipSuccess) {
            if (ek.second == 0) { h->roll_ms += ms; h->roll_n++; }
            else if (ek.second == 1) h->sel_ms += ms;
            else if (ek.second == 2) h->red_ms += ms;
            else h->samp_ms += ms;
        }
    }
    h->ev_kind.clear();
}

// ---- warm start (cem_mpc.h: cem_init_mode) ---------------------------------------------------------------
// The host owns the bookkeeping (which slot's carry is valid, where it currently lives), the first kernel of a plan does the copies.
// A plan's last mu / sigma stay where the select left them — slice b of Layout::musig — until the NEXT plan's first kernel, which is
// about to restart every slice, moves them to the slot's carry first (WarmProb::save_slot).  Nothing else touches Layout::musig between
// two plans, and that kernel is ordered behind the whole previous plan by the stream, early stop or not.
// (by the bits: the library is built with -fno-honor-nans, under which the compiler may drop a floating-point NaN test)
bool finite_bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return (u & 0x7f800000u) != 0x7f800000u; }

// what has to hold before anything of a plan of n problems is staged
int check_warm(const cem_planner *h, int n)
{
    for (int b = 0; b < n; ++b) {
        const int s = h->slot_of[b];
        if (h->slot_mode[s] == CEM_INIT_EXPLICIT && !h->have_expl[s]) return CEM_ERR_STATE;
    }
    return CEM_OK;
}

// INVARIANT: the hand-over of a pending carry (carry_at[s] -> WarmProb::save_slot) is consumed by exactly one EXECUTED first kernel.
// stage_warm only describes it and may run any number of times before a launch (a plan whose capture fails is staged once, but between
// staging and launch a HIP call may fail, and the next plan is staged over it): it rebuilds save_slot from carry_at and changes
// nothing.  warm_handed_over, called at the two places the first kernel is really put on the stream (enqueue_begin outside a capture,
// run_plan's graph launch), is what clears carry_at — from then on the carries are in Layout::carry, in stream order, and a later staging (a second
// cem_plan_begin without an end, say) must not save the slices again, which hold the new plan's distribution by then.
void warm_handed_over(cem_planner *h)
{
    for (auto &c : h->carry_at) c = -1;
    if (h->warm_save_skipped) { h->carry_valid[0] = 0; h->warm_save_skipped = false; }   // (stage_warm: the launched plan overwrites a carry nobody copied)
}

void stage_warm(cem_planner *h, int n)
{
    WarmCtl *w = h->h_warm;
    const int nb = warm_slots(h);
    w->shift = h->warm.shift; w->tail = h->warm.tail; w->sigma_rule = h->warm.sigma_rule;
    for (int a = 0; a < 32; ++a) w->sigma_floor[a] = h->warm.sigma_floor[a];
    for (int b = 0; b < nb; ++b) { w->prob[b].mode = CEM_INIT_COLD; w->prob[b].slot = h->slot_of[b]; w->prob[b].save_slot = -1; w->prob[b].pad = 0; }
    for (int s = 0; s < nb; ++s)                                   // carries still in a mu / sigma slice: all of them move now, also
        if (h->carry_at[s] >= 0) w->prob[h->carry_at[s]].save_slot = s;                            // those of slots that sit this plan out
    w->two_phase = 0;
    for (int b = 0; b < n; ++b) {
        const int s = h->slot_of[b];
        int m = h->slot_mode[s];
        if (m == CEM_INIT_SHIFT && !h->carry_valid[s]) m = CEM_INIT_COLD;
        w->prob[b].mode = m;
        if (m == CEM_INIT_SHIFT) w->two_phase = 1;            // some problem reads a carry: the first kernel takes its two-phase form
    }
    // A single-state handle whose plan does not read the carry needs no copy of it either: the plan overwrites the one slice there is, and
    // until its own result becomes the carry nothing can read the old one (cem_planner_get_carry is refused inside a stepwise plan; the
    // launch drops the old carry's validity, see warm_handed_over).  This keeps a cold plan's first kernel free of loads.
    h->warm_save_skipped = !h->batch && !w->two_phase && w->prob[0].save_slot >= 0;
    if (h->warm_save_skipped) w->prob[0].save_slot = -1;
    h->warm_staged = n;
}

// the plan staged last has returned `status`: its slots' carries are what it left (CEM_OK) or invalid
void finish_warm(cem_planner *h, int status)
{
    for (int b = 0; b < h->warm_staged; ++b) {
        const int s = h->slot_of[b];
        h->carry_valid[s] = status == CEM_OK; h->carry_at[s] = status == CEM_OK ? b : -1;
    }
    h->warm_staged = 0;
}

// One plan call as every entry point describes it: n problems side by side (cem_planner_plan, cem_plan_begin: one), problem b with state
// states[b][O], Philox key (seed, calls[b]) and row b of the outputs.  eps_act / eps_model: device tensors or null; eps_out: host or null.
struct PlanCall {
    int n; const float *states; uint64_t seed; const uint64_t *calls;
    const float *eps_act, *eps_model, *eps_out;
    float *actions, *scores; int32_t *iters;
};

// explicit noise comes as both tensors or neither (the sampler of the propagation draws from both)
bool noise_pair_ok(const cem_planner *h, const PlanCall &pc)
{
    return (pc.eps_act == nullptr) == (pc.eps_model == nullptr) || !h->cfg.sampling_propagation;
}

// The plan's control blocks, one per problem of the handle: problem b < n gets states[b] and the key (seed, calls[b]) — what a
// single-state handle stages for that state alone; problems n .. batch - 1 are staged as already stopped (done, no iterations), so every
// kernel skips them.  Runs once per plan a caller sees: the plan counter advances by one.
void stage_ctrl(cem_planner *h, const PlanCall &pc)
{
    stage_warm(h, pc.n);
    const uint32_t seq = ++h->plan_seq;                  // echoed into result[36] by the kernel that completes the plan
    for (int b = 0; b < warm_slots(h); ++b) {
        CtrlBlock *c = h->h_ctrl + b;
        const bool live = b < pc.n;
        const uint64_t call = live ? pc.calls[b] : 0;
        c->seed_lo = (uint32_t)pc.seed; c->seed_hi = (uint32_t)(pc.seed >> 32); c->call_lo = (uint32_t)call; c->call_hi = (uint32_t)(call >> 32);
        c->done = live ? 0 : 1; c->iters = 0; c->fault = 0; c->best_score = -std::numeric_limits<float>::infinity();
        for (int f = 0; f < CEM_U; ++f) c->state[f] = (live && f < h->d.O) ? pc.states[(size_t)b * h->d.O + f] : 0.f;
        for (int a = 0; a < 32; ++a) c->best[a] = 0.f;
        c->seq = seq; c->inject = h->batch ? 0 : h->inject_next;     // (test hook, cem_planner_inject_fault: single-state handles consume it)
    }
    if (!h->batch) h->inject_next = 0;
    h->n_states = pc.n;
}

// The plan is queued: wait for its result.  The kernel that completes it stores the plan counter into pinned host memory after
// everything else of the result, so the host watches that word — a few hundred nanoseconds after the store — instead of going
// through hipStreamSynchronize (an interrupt / yield path that took ~10 us of a 1.9-ms plan).  Bounded: after 100 ms of polling the
// ordinary synchronisation takes over.
// the block is complete when it carries this plan's counter AND its checksum holds (device -> host writes arrive in no particular order)
// (every block of the plan's problems, [n_states][CEM_RESULT_WORDS]; a single-state handle has the one)
bool result_landed(const cem_planner *h)
{
    for (int b = 0; b < h->n_states; ++b) {
        const volatile uint32_t *r = reinterpret_cast<const volatile uint32_t *>(h->h_result) + (size_t)b * CEM_RESULT_WORDS;
        if (r[36] != h->plan_seq) return false;
        if (cem_result_checksum(r, h->plan_seq) != r[37]) return false;     // position dependent: stale words cannot cancel (cem_device.h)
    }
    return true;
}

int wait_result(cem_planner *h)
{
    // CEM_NO_POLL: a host that would rather sleep than spin a core for the ~2 ms of a plan goes straight to the stream synchronisation
    static const bool no_poll = std::getenv("CEM_NO_POLL") != nullptr;
    if (!no_poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 1;; ++spin) {
            if (result_landed(h)) { std::atomic_thread_fence(std::memory_order_acquire); return CEM_OK; }
#if defined(__x86_64__)
            __builtin_ia32_pause();
#endif
            if ((spin & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(100)) break;   // a plan that long is not latency-critical; a faulted device never writes the block
        }
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

// the results of the plan's n problems: row b of the outputs from block b
int read_results(cem_planner *h, const PlanCall &pc)
{
    // (after a stream synchronisation the blocks have landed; the check costs nothing and a short wait covers a write still in flight)
    for (int spin = 0; spin < 2000000 && !result_landed(h); ++spin) { }
    if (!result_landed(h)) return CEM_ERR_DEVICE;
    int32_t fault = 0;
    for (int b = 0; b < pc.n; ++b) {
        const float *r = h->h_result + (size_t)b * CEM_RESULT_WORDS;
        if (pc.actions) std::memcpy(pc.actions + (size_t)b * h->d.A, r, h->d.A * 4);
        if (pc.scores) pc.scores[b] = r[32];
        if (pc.iters) pc.iters[b] = reinterpret_cast<const int32_t *>(r)[33];
        fault |= reinterpret_cast<const int32_t *>(r)[35];                                  // CtrlBlock::fault
    }
    if (fault & CEM_FAULT_RECOVERED) {                  // (the fused select only: never on a batch handle, which runs the one-workgroup select)
        // A grid barrier of the fused select expired (its workgroups were not all resident: another stream, handle or process held
        // CUs) and cem_msel_solo_kernel redid that iteration's select in stream order: the plan is valid, with select_mode 2's bits.
        // This handle stops fusing: the next plan re-captures its graph on the eight-launch chain, which has no residency assumption.
        if (!h->fuse_banned) {
            std::fprintf(stderr, "cem_mpc: a grid barrier of the fused select timed out (GPU shared with other work?); that iteration's select was redone "
                                 "by the recovery kernel and this handle uses the multi-launch select (select_mode 2) from now on\n");
            h->fuse_banned = true;
            if (hipStreamSynchronize(h->stream) != hipSuccess) (void)hipGetLastError();      // the graph may still be draining behind the polled result
            drop_graph(h);
        }
    }
    return (fault & (CEM_FAULT_SEGMENT | CEM_FAULT_BARRIER)) ? CEM_ERR_DEVICE : CEM_OK;     // a kernel gave up and nothing made up for it
}

// A whole plan recorded on the stream — under capture and eagerly alike; the one place the iteration loop exists.  The first kernel,
// then per iteration rollout, exchange (a no-op without a communicator) and select, then the final kernel unless the last select wrote
// the result itself (single-state handles on the one-workgroup select: enqueue_select).
int enqueue_plan(cem_planner *h, bool have_eps_out)
{
    bool final_folded = false;
    int st = enqueue_begin(h);
    for (int it = 0; it < h->d.I && !st; ++it) {
        st = enqueue_rollout(h, it, true);
        if (!st) st = enqueue_exchange(h);
        if (!st) st = enqueue_select(h, it, true, have_eps_out, &final_folded);
    }
    if (!st && !final_folded) st = enqueue_end(h, have_eps_out);
    return st;
}

// The handle's hipGraph: the staged plan captured once (for all `batch` problems of a batch handle: n_states only changes what is staged,
// never the graph) and kept until something drops it.  Leaves graph_ready set, or — CEM_OK all the same — graph_failed: a captured
// collective is not something every RCCL / runtime pair supports, so a handle with a communicator whose capture does not work launches
// eagerly for good, as does one told so by cem_planner_inject_fault(h, 2).  Without either the failure is the caller's; batch handles
// never fall back.
int ensure_graph(cem_planner *h)
{
    if (h->graph_ready) return CEM_OK;
    h->eps_act = h->eps_model = nullptr;
    // relaxed mode: RCCL may touch the runtime from its proxy thread while this thread captures
    HIPCHK(hipStreamBeginCapture(h->stream, h->comm ? hipStreamCaptureModeRelaxed : hipStreamCaptureModeThreadLocal));
    const int st = enqueue_plan(h, false);
    hipError_t ce = hipStreamEndCapture(h->stream, &h->graph);
    if (!st && ce == hipSuccess) ce = hipGraphInstantiate(&h->gexec, h->graph, nullptr, nullptr, 0);
    const bool refuse = !h->batch && h->inject_capture_fail;       // (test hook, cem_planner_inject_fault kind 2)
    if (!h->batch) h->inject_capture_fail = false;
    if (!st && ce == hipSuccess && !refuse) { h->graph_ready = true; return CEM_OK; }
    if (st || ce != hipSuccess) h->gexec = nullptr;                // (nothing was instantiated)
    drop_graph(h);
    if (!h->comm && !refuse) { if (st) return st; HIPCHK(ce); }
    (void)hipGetLastError();
    h->graph_failed = true;
    return CEM_OK;
}

// the counts of the elite stores go back to zero in front of a plan that follows a failed one (outside any capture)
int clear_elite_after_failure(cem_planner *h)
{
    if (h->elite_clear && h->elite_dev) HIPCHK(hipMemsetAsync(elite_counts(h), 0, (size_t)warm_slots(h) * 4, h->stream));
    h->elite_clear = false;
    return CEM_OK;
}

// The one plan driver, behind cem_planner_plan (one problem) and cem_planner_plan_batch alike; the entry points have checked their
// arguments.  Stage, then replay the graph or launch the same kernels eagerly, wait, read the n results.
int run_plan(cem_planner *h, const PlanCall &pc)
{
    // With a communicator the first plan runs eagerly: RCCL finishes its lazy set-up (buffers, kernels) outside any capture.
    bool graph = h->cfg.use_graph && !pc.eps_act && !pc.eps_model && !pc.eps_out && !h->timing && !h->graph_failed &&
                 (!h->comm || h->plans_since_comm > 0);
    if (h->comm) h->plans_since_comm++;
    { const int wst = check_warm(h, pc.n); if (wst) return wst; }
    if (!noise_pair_ok(h, pc)) return CEM_ERR_INVALID_ARG;
    stage_ctrl(h, pc);
    { const int est = clear_elite_after_failure(h); if (est) return est; }
    if (h->opt.cost_m) note_plan_cstat(h);
    if (graph) { const int st = ensure_graph(h); if (st) return st; graph = h->graph_ready; }
    if (graph) {
        HIPCHK(hipGraphLaunch(h->gexec, h->stream));
        warm_handed_over(h);                            // the graph's first kernel is on the stream (the eager one: enqueue_begin)
        const int st = wait_result(h); if (st) return st;
    } else {
        if (pc.eps_out) HIPCHK(hipMemcpyAsync(h->ws + h->lay.eps_out, pc.eps_out, (size_t)pc.n * h->d.A * 4, hipMemcpyHostToDevice, h->stream));
        h->eps_act = pc.eps_act; h->eps_model = pc.eps_model;
        h->ev_kind.clear();
        const int st = enqueue_plan(h, pc.eps_out != nullptr);
        h->eps_act = h->eps_model = nullptr;
        if (st) return st;
        HIPCHK(hipStreamSynchronize(h->stream));
        if (h->timing) collect_timing(h);
    }
    return read_results(h, pc);
}

// Whatever a plan whose control data was staged returns decides whether its slots' carries are valid (finish_warm); a call refused
// before staging leaves them alone.
int settle_warm(cem_planner *h, int status)
{
    if (h && status != CEM_OK) h->elite_clear = true;     // (cem_elite_carry.h: nothing of a plan call that failed is carried into the next plan)
    if (h && h->warm_staged) finish_warm(h, status);
    return status;
}

}  // namespace

extern "C" {

// The public plan calls.  Each makes its own checks, in its own order (which status a bad call gets is part of the contract), and hands the
// rest to run_plan; whatever comes back settles the carries (settle_warm).
int cem_planner_plan_batch(cem_planner_t *h, int32_t n_states, const float *states, uint64_t seed, const uint64_t *calls,
                           const float *eps_act_dev, const float *eps_model_dev, const float *eps_out_host, float *actions_out,
                           float *best_scores_out, int32_t *iters_out)
{
    const PlanCall pc{n_states, states, seed, calls, eps_act_dev, eps_model_dev, eps_out_host, actions_out, best_scores_out, iters_out};
    const int st = !h ? CEM_ERR_INVALID_ARG
                 : !h->batch ? CEM_ERR_STATE                                 // a single-state handle: cem_planner_plan
                 : (!states || !calls || n_states < 1 || n_states > h->batch) ? CEM_ERR_INVALID_ARG
                 : !h->have_weights ? CEM_ERR_NO_WEIGHTS
                 : !noise_pair_ok(h, pc) ? CEM_ERR_INVALID_ARG               // (this entry: ahead of the warm-start check)
                 : run_plan(h, pc);
    return settle_warm(h, st);
}

int cem_planner_plan(cem_planner_t *h, const float *state, uint64_t seed, uint64_t call, const float *eps_act_dev,
                     const float *eps_model_dev, const float *eps_out_host, float *action_out, float *best_score_out, int32_t *iters_out)
{
    const PlanCall pc{1, state, seed, &call, eps_act_dev, eps_model_dev, eps_out_host, action_out, best_score_out, iters_out};
    const int st = (!h || !state) ? CEM_ERR_INVALID_ARG
                 : h->batch ? CEM_ERR_STATE                                  // a batch handle plans through cem_planner_plan_batch only
                 : !h->have_weights ? CEM_ERR_NO_WEIGHTS
                 : (h->d.W != 1 && !h->comm) ? CEM_ERR_STATE                 // sharded ranks without cem_planner_comm_init use the stepwise calls around their own collective
                 : run_plan(h, pc);
    return settle_warm(h, st);
}

// The stepwise form of a single-state plan: the same launches, one call each, the scores left in scores_local between rollout and select
// (the caller may exchange them).
static int plan_begin_impl(cem_planner_t *h, const float *state, uint64_t seed, uint64_t call, const float *eps_act_dev, const float *eps_model_dev)
{
    if (!h || !state) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;                  // a batch handle plans through cem_planner_plan_batch only
    if (!h->have_weights) return CEM_ERR_NO_WEIGHTS;
    const PlanCall pc{1, state, seed, &call, eps_act_dev, eps_model_dev, nullptr, nullptr, nullptr, nullptr};
    if (!noise_pair_ok(h, pc)) return CEM_ERR_INVALID_ARG;
    { const int wst = check_warm(h, 1); if (wst) return wst; }
    stage_ctrl(h, pc);
    { const int est = clear_elite_after_failure(h); if (est) return est; }
    h->eps_act = eps_act_dev; h->eps_model = eps_model_dev;
    h->ev_kind.clear();
    int st = enqueue_begin(h); if (st) return st;
    h->in_plan = true;
    return CEM_OK;
}

int cem_plan_begin(cem_planner_t *h, const float *state, uint64_t seed, uint64_t call, const float *eps_act_dev, const float *eps_model_dev)
{
    const int st = plan_begin_impl(h, state, seed, call, eps_act_dev, eps_model_dev);
    return st ? settle_warm(h, st) : st;                 // (a plan that began is settled by its end call)
}

int cem_plan_rollout(cem_planner_t *h, int32_t it)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (!h->in_plan) return CEM_ERR_STATE;
    if (it < 0 || it >= h->d.I) return CEM_ERR_INVALID_ARG;
    return enqueue_rollout(h, it, false);
}

int cem_plan_select(cem_planner_t *h, int32_t it)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (!h->in_plan) return CEM_ERR_STATE;
    if (!h->pop.empty() && (it < 0 || it >= h->d.I)) return CEM_ERR_INVALID_ARG;     // (a scheduled select needs to know whose population it ranks)
    return enqueue_select(h, it, false);
}

static int plan_end_impl(cem_planner_t *h, const float *eps_out_host, float *action_out, float *best_score_out, int32_t *iters_out)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (!h->in_plan) return CEM_ERR_STATE;
    h->in_plan = false;
    if (eps_out_host) HIPCHK(hipMemcpyAsync(h->ws + h->lay.eps_out, eps_out_host, h->d.A * 4, hipMemcpyHostToDevice, h->stream));
    int st = enqueue_end(h, eps_out_host != nullptr); if (st) return st;
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->timing) collect_timing(h);
    const PlanCall pc{1, nullptr, 0, nullptr, nullptr, nullptr, eps_out_host, action_out, best_score_out, iters_out};
    return read_results(h, pc);
}

int cem_plan_end(cem_planner_t *h, const float *eps_out_host, float *action_out, float *best_score_out, int32_t *iters_out)
{
    const int st = plan_end_impl(h, eps_out_host, action_out, best_score_out, iters_out);
    return (h && !h->in_plan) ? settle_warm(h, st) : st;
}

int cem_planner_set_warm_start(cem_planner_t *h, const cem_warm_start_t *ws)
{
    if (!h || !ws) return CEM_ERR_INVALID_ARG;
    if (ws->shift < 1 || ws->shift >= h->d.H || (ws->tail != 0 && ws->tail != 1) || (ws->sigma_rule != 0 && ws->sigma_rule != 1)) return CEM_ERR_INVALID_ARG;
    for (int a = 0; a < h->d.A; ++a) if (!finite_bits(ws->sigma_floor[a]) || ws->sigma_floor[a] < 0.f) return CEM_ERR_INVALID_ARG;
    h->warm = *ws;
    for (int a = h->d.A; a < CEM_MAX_ACT; ++a) h->warm.sigma_floor[a] = 0.f;
    return CEM_OK;
}

int cem_planner_set_particle_objective(cem_planner_t *h, int32_t kind, int32_t m)
{
    if (!h || (kind != CEM_PARTICLES_MEAN && kind != CEM_PARTICLES_LOWER_TAIL)) return CEM_ERR_INVALID_ARG;
    if (kind == CEM_PARTICLES_LOWER_TAIL && (m < 1 || m > h->d.P)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.tail_m = kind == CEM_PARTICLES_LOWER_TAIL ? m : 0;
    { const int st = admit_on(h, next); if (st) return st; }
    if (next.tail_m == h->opt.tail_m) return CEM_OK;
    // the captured plan holds the other objective's launches (and, changing m alone, the old m): the next plan captures anew
    return commit_launch_change(h, next, false);
}

int cem_planner_get_particle_objective(const cem_planner_t *h, int32_t *kind_out, int32_t *m_out)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (kind_out) *kind_out = h->opt.tail_m ? CEM_PARTICLES_LOWER_TAIL : CEM_PARTICLES_MEAN;
    if (m_out) *m_out = h->opt.tail_m;
    return CEM_OK;
}

// the handle's budget allocation (cem_planner::budget_dev), made on first use: the budgets as the host copy holds them, cstat zeroed
static int ensure_budget(cem_planner *h)
{
    if (h->budget_dev) return CEM_OK;
    const size_t nb = (size_t)warm_slots(h), floats = nb + nb * (size_t)h->d.Nloc;
    HIPCHK(hipMalloc((void **)&h->budget_dev, floats * 4));
    HIPCHK(hipMemsetAsync(h->budget_dev, 0, floats * 4, h->stream));
    HIPCHK(hipMemcpyAsync(h->budget_dev, h->h_budget.data(), nb * 4, hipMemcpyHostToDevice, h->stream));
    return CEM_OK;
}

int cem_planner_set_constraint(cem_planner_t *h, int32_t kind, int32_t worst_cost_particles)
{
    if (!h || (kind != CEM_CONSTRAINT_BETA && kind != CEM_CONSTRAINT_BUDGET)) return CEM_ERR_INVALID_ARG;
    if (kind == CEM_CONSTRAINT_BUDGET && (worst_cost_particles < 0 || worst_cost_particles > h->d.P)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.cost_m = kind != CEM_CONSTRAINT_BUDGET ? 0 : worst_cost_particles ? worst_cost_particles : h->d.P;
    { const int st = admit_on(h, next); if (st) return st; }
    if (next.cost_m == h->opt.cost_m) return CEM_OK;
    // the captured plan holds the other constraint's launches (and, changing m_c alone, the old m_c): the next plan captures anew
    if (next.cost_m) { const int st = ensure_budget(h); if (st) return st; }
    return commit_launch_change(h, next, false);
}

int cem_planner_get_constraint(const cem_planner_t *h, int32_t *kind_out, int32_t *worst_cost_particles_out)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (kind_out) *kind_out = h->opt.cost_m ? CEM_CONSTRAINT_BUDGET : CEM_CONSTRAINT_BETA;
    if (worst_cost_particles_out) *worst_cost_particles_out = h->opt.cost_m;
    return CEM_OK;
}

int cem_planner_set_cost_budget(cem_planner_t *h, const float *budgets, int32_t n)
{
    if (!h || !budgets || n < 1 || n > warm_slots(h)) return CEM_ERR_INVALID_ARG;
    for (int i = 0; i < n; ++i) { uint32_t u; std::memcpy(&u, &budgets[i], 4); if ((u & 0x7fffffffu) > 0x7f800000u) return CEM_ERR_INVALID_ARG; }   // NaN, by its bits (-fno-honor-nans)
    if (h->in_plan) return CEM_ERR_STATE;
    const int st = ensure_budget(h); if (st) return st;
    // through a copy the handle owns (as cem_planner_set_initial_distribution): the caller's array need not outlive this call
    const int rows = n == 1 ? warm_slots(h) : n;
    for (int i = 0; i < rows; ++i) h->h_budget[i] = budgets[n == 1 ? 0 : i];
    HIPCHK(hipMemcpyAsync(h->budget_dev, h->h_budget.data(), (size_t)rows * 4, hipMemcpyHostToDevice, h->stream));
    return CEM_OK;
}

int cem_planner_constraint_costs(cem_planner_t *h, int32_t problem, float *out_host, int32_t n)
{
    if (!h || !out_host || n < 1 || problem < 0) return CEM_ERR_INVALID_ARG;
    if (!h->last_cstat) return CEM_ERR_STATE;
    if (problem >= std::max(h->last_cstat_problems, 1) || n > h->last_cstat_n) return CEM_ERR_INVALID_ARG;
    HIPCHK(hipStreamSynchronize(h->stream));
    HIPCHK(hipMemcpy(out_host, h->last_cstat + (size_t)problem * h->last_cstat_n, (size_t)n * 4, hipMemcpyDeviceToHost));
    return CEM_OK;
}

// the handle's refit allocation (cem_planner::refit_dev), made on first use and zeroed: the scratch slices the select of a weighted
// iteration blends into (finite from the start, so they stay finite), then the ESS rows
static int ensure_refit(cem_planner *h)
{
    if (h->refit_dev) return CEM_OK;
    const size_t floats = (size_t)warm_slots(h) * (2 * (size_t)h->d.H * h->d.A + (size_t)h->d.I);
    // the weights of up to 24576 elites: beyond the default 64 KB of dynamic LDS the runtime has to be asked (as the select kernels are, at create)
    if (CEM_REFIT_LDS_BYTES(h->d.k, h->d.H * h->d.A) > 48 * 1024)
        HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_constraint_refit_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 140 * 1024));
    HIPCHK(hipMalloc((void **)&h->refit_dev, floats * 4));
    HIPCHK(hipMemsetAsync(h->refit_dev, 0, floats * 4, h->stream));
    return CEM_OK;
}

int cem_planner_set_refit(cem_planner_t *h, int32_t kind, float temperature)
{
    if (!h || (kind != CEM_REFIT_UNIFORM && kind != CEM_REFIT_SOFTMAX)) return CEM_ERR_INVALID_ARG;
    if (kind == CEM_REFIT_SOFTMAX && (!finite_bits(temperature) || !(temperature > 0.f))) return CEM_ERR_INVALID_ARG;   // (NaN: by its bits, -fno-honor-nans)
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.refit_kind = kind; next.refit_tau = kind == CEM_REFIT_SOFTMAX ? temperature : 0.f;
    { const int st = admit_on(h, next, PLAN_CHANGE_REFIT); if (st) return st; }
    if (kind == h->opt.refit_kind && std::memcmp(&next.refit_tau, &h->opt.refit_tau, 4) == 0) return CEM_OK;
    // the captured plan holds the other refit's launches (and, changing the temperature alone, the old 1 / temperature): the next plan captures anew
    if (kind == CEM_REFIT_SOFTMAX) { const int st = ensure_refit(h); if (st) return st; }
    return commit_launch_change(h, next, false, [&] { h->refit_beta = kind == CEM_REFIT_SOFTMAX ? 1.0f / temperature : 0.f; return (int)CEM_OK; });
}

int cem_planner_get_refit(const cem_planner_t *h, int32_t *kind_out, float *temperature_out)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (kind_out) *kind_out = h->opt.refit_kind;
    if (temperature_out) *temperature_out = h->opt.refit_tau;
    return CEM_OK;
}

int cem_planner_refit_stats(cem_planner_t *h, int32_t problem, float *ess_out_host, int32_t n)
{
    if (!h || !ess_out_host || n < 1 || problem < 0) return CEM_ERR_INVALID_ARG;
    if (problem >= warm_slots(h) || n > h->d.I) return CEM_ERR_INVALID_ARG;
    if (!h->refit_ran) return CEM_ERR_STATE;
    HIPCHK(hipStreamSynchronize(h->stream));
    const float *stat = h->refit_dev + (size_t)warm_slots(h) * 2 * h->d.H * h->d.A + (size_t)problem * h->d.I;
    HIPCHK(hipMemcpy(ess_out_host, stat, (size_t)n * 4, hipMemcpyDeviceToHost));
    return CEM_OK;
}

int cem_planner_set_action_noise(cem_planner_t *h, int32_t kind, const float *mix_host)
{
    if (!h || (kind != CEM_NOISE_WHITE && kind != CEM_NOISE_MIXED)) return CEM_ERR_INVALID_ARG;
    if ((kind == CEM_NOISE_MIXED) != (mix_host != nullptr)) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    const size_t HH = (size_t)d.H * d.H;
    if (kind == CEM_NOISE_MIXED) for (size_t i = 0; i < HH; ++i) if (!finite_bits(mix_host[i])) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.noise_kind = kind;
    { const int st = admit_on(h, next); if (st) return st; }
    if (kind == CEM_NOISE_WHITE && h->opt.noise_kind == CEM_NOISE_WHITE) return CEM_OK;
    // the handle's noise allocation (cem_planner::noise_dev), made on first use and zeroed: M transposed, then the mixed tensor of every
    // slot.  A handle this call fails on keeps what it had (cem_planner_action_noise_dev reports NULL on one that has never been MIXED)
    const size_t mt = (HH + 3) & ~(size_t)3, eps = (size_t)warm_slots(h) * d.I * d.N * d.H * d.A;
    DevBlock made;
    if (kind == CEM_NOISE_MIXED && !h->noise_dev) {
        HIPCHK(prepare_mix_action_noise(d.H));
        HIPCHK(made.alloc((mt + eps) * 4));
        HIPCHK(hipMemsetAsync(made.p, 0, (mt + eps) * 4, h->stream));
    }
    // The wait is unconditional — not only for a captured plan, as in the sibling setters: an EAGER MIXED plan still draining behind its
    // polled result may be reading the matrix about to be overwritten.
    return commit_launch_change(h, next, true, [&]() -> int {
        if (kind != CEM_NOISE_MIXED) return CEM_OK;
        std::vector<float> mix(mix_host, mix_host + HH), mix_t(HH);
        for (int t = 0; t < d.H; ++t) for (int u = 0; u < d.H; ++u) mix_t[(size_t)u * d.H + t] = mix_host[(size_t)t * d.H + u];
        // (the swap below keeps mix_t's storage alive in the handle for as long as the stream may read it)
        HIPCHK(hipMemcpyAsync(made.p ? made.p : h->noise_dev, mix_t.data(), HH * 4, hipMemcpyHostToDevice, h->stream));
        if (made.p) { h->noise_dev = made.release<float>(); h->noise_eps = h->noise_dev + mt; h->noise_floats = eps; }
        h->h_mix.swap(mix); h->h_mix_t.swap(mix_t);
        return CEM_OK;
    });
}

int cem_planner_get_action_noise(const cem_planner_t *h, int32_t *kind_out, float *mix_out_host)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (kind_out) *kind_out = h->opt.noise_kind;
    if (mix_out_host && h->opt.noise_kind == CEM_NOISE_MIXED) std::memcpy(mix_out_host, h->h_mix.data(), h->h_mix.size() * 4);
    return CEM_OK;
}

int cem_planner_action_noise_dev(cem_planner_t *h, const float **eps_dev_out, size_t *n_floats_out)
{
    if (!h || !eps_dev_out || !n_floats_out) return CEM_ERR_INVALID_ARG;
    *eps_dev_out = h->noise_eps; *n_floats_out = h->noise_floats;
    return CEM_OK;
}

int cem_planner_set_elite_carry(cem_planner_t *h, const cem_elite_carry_t *ec)
{
    if (!h || !ec) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    if (ec->n_keep < 0 || ec->n_keep > d.k || ec->n_keep >= d.N) return CEM_ERR_INVALID_ARG;
    if ((ec->across_plans != 0 && ec->across_plans != 1) || ec->reserved != 0) return CEM_ERR_INVALID_ARG;
    if (ec->across_plans && (ec->shift < 1 || ec->shift >= d.H)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.elite = *ec;
    { const int st = admit_on(h, next); if (st) return st; }
    // a larger store is allocated before anything of the handle changes: a failed allocation leaves it as it was
    DevBlock grown;
    const size_t HA = (size_t)d.H * d.A, floats = elite_count_floats(h) + (size_t)warm_slots(h) * ec->n_keep * HA;
    if (ec->n_keep > h->elite_cap) HIPCHK(grown.alloc(floats * 4));
    // Unconditional, as in cem_planner_set_action_noise: an eager plan still draining behind its polled result may be reading the store
    return commit_launch_change(h, next, true, [&]() -> int {
        if (grown.p) {
            HIPCHK(hipMemsetAsync(grown.p, 0, floats * 4, h->stream));
            if (h->elite_dev) hipFree(h->elite_dev);
            h->elite_dev = grown.release<float>(); h->elite_cap = ec->n_keep;
        } else if (h->elite_dev) HIPCHK(hipMemsetAsync(elite_counts(h), 0, (size_t)warm_slots(h) * 4, h->stream));   // every call empties the stores
        h->elite_clear = false;
        return CEM_OK;
    });
}

int cem_planner_set_plan_readout(cem_planner_t *h, int32_t enable)
{
    if (!h || (enable != 0 && enable != 1)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    const Dims &d = h->d;
    PlanOptions next = options_of(h); next.readout = enable;
    { const int st = admit_on(h, next); if (st) return st; }
    // the blocks are allocated before anything of the handle changes: a failed allocation leaves it as it was
    DevBlock made;
    const size_t stride = CEM_READOUT_WORDS(d.H, d.A, d.P), words = (size_t)warm_slots(h) * stride;
    if (enable && !h->readout_dev) HIPCHK(made.alloc(words * 4));
    // Unconditional, as in cem_planner_set_elite_carry: an eager plan still draining behind its polled result may be writing the blocks
    return commit_launch_change(h, next, true, [&]() -> int {
        if (!made.p) return CEM_OK;
        // every block starts as the tracker's reset leaves it: a read-out asked for before any plan says "nothing found"
        std::vector<uint32_t> init(words, 0u);
        for (int b = 0; b < warm_slots(h); ++b) {
            uint32_t *blk = init.data() + (size_t)b * stride;
            blk[0] = 0xff800000u; blk[1] = 0xffffffffu; blk[2] = 0xffffffffu;
            if (h->cfg.variant == CEM_VARIANT_CEM) for (int t = 0; t < d.H; ++t) blk[stride - d.H + t] = 0xffffffffu;
        }
        HIPCHK(hipMemcpy(made.p, init.data(), words * 4, hipMemcpyHostToDevice));
        h->readout_dev = made.release<uint32_t>();
        return CEM_OK;
    });
}

int cem_planner_get_plan_readout(const cem_planner_t *h, int32_t *enable_out)
{
    if (!h || !enable_out) return CEM_ERR_INVALID_ARG;
    *enable_out = h->opt.readout;
    return CEM_OK;
}

int cem_planner_plan_readout(cem_planner_t *h, int32_t problem, cem_plan_readout_t *out, float *sequence_out_host,
                             float *particle_returns_out_host, int32_t *cost_counts_out_host)
{
    if (!h || !out || problem < 0 || problem >= warm_slots(h)) return CEM_ERR_INVALID_ARG;
    if (!h->opt.readout || !h->readout_dev) return CEM_ERR_STATE;
    // the last iteration's tracker runs BEHIND the select that hands the polled result to the host: the stream is drained first
    HIPCHK(hipStreamSynchronize(h->stream));
    const Dims &d = h->d;
    const size_t HA = (size_t)d.H * d.A;
    const uint32_t *blk = h->readout_dev + (size_t)problem * CEM_READOUT_WORDS(d.H, d.A, d.P);
    uint32_t head[CEM_READOUT_HEAD];
    HIPCHK(hipMemcpy(head, blk, sizeof head, hipMemcpyDeviceToHost));
    std::memcpy(&out->score, &head[0], 4); out->candidate = (int32_t)head[1]; out->iteration = (int32_t)head[2]; out->flags = (int32_t)head[3];
    if (sequence_out_host) HIPCHK(hipMemcpy(sequence_out_host, blk + CEM_READOUT_HEAD, HA * 4, hipMemcpyDeviceToHost));
    if (particle_returns_out_host) HIPCHK(hipMemcpy(particle_returns_out_host, blk + CEM_READOUT_HEAD + HA, (size_t)d.P * 4, hipMemcpyDeviceToHost));
    if (cost_counts_out_host) HIPCHK(hipMemcpy(cost_counts_out_host, blk + CEM_READOUT_HEAD + HA + d.P, (size_t)d.H * 4, hipMemcpyDeviceToHost));
    return CEM_OK;
}

// cem_planner_set_task (trk null) and cem_planner_set_task_tracking (task: its base; cem_task_reference.h), which differ in the second
// table row (g / qT), in the kind and in what the tracking task owns besides: the reference table and the clock
static int set_task(cem_planner_t *h, const cem_task_t *task, const cem_task_tracking_t *trk)
{
    const Dims &d = h->d;
    const bool on = task && task->kind != CEM_TASK_SAFETY_GYM;
    // on the bit patterns: this file is built with -fno-honor-nans
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    auto finite = [&](float v) { return (bits(v) & 0x7fffffffu) < 0x7f800000u; };
    auto is_nan = [&](float v) { return (bits(v) & 0x7fffffffu) > 0x7f800000u; };
    // the tables as the kernel reads them: [CEM_TASK_TABLES][CEM_U], the defaults beyond obs_dim and for a NULL table
    std::vector<float> tab(task_tab_floats(), 0.f);
    TaskParams tp{};
    float kappa[CEM_MAX_ACT] = {};
    std::vector<uint32_t> trk_host;                            // the clock block at (0, zeros), then ref as the kernel reads it: [T][CEM_U], zero beyond obs_dim
    if (on) {
        const float inf = std::numeric_limits<float>::infinity();
        const float *src[CEM_TASK_TABLES] = {task->q, trk ? (trk->q_terminal ? trk->q_terminal : task->q) : task->g, task->c, task->goal_mask, task->lo, task->hi};
        for (int f = 0; f < CEM_U; ++f) { tab[CEM_TASK_TAB_LO * CEM_U + f] = -inf; tab[CEM_TASK_TAB_HI * CEM_U + f] = inf; }
        for (int k = 0; k < CEM_TASK_TABLES; ++k)
            for (int f = 0; src[k] && f < d.O; ++f) {
                const float v = src[k][f];
                if (k < CEM_TASK_TAB_LO ? !finite(v) : is_nan(v)) return CEM_ERR_INVALID_ARG;
                tab[(size_t)k * CEM_U + f] = v;
            }
        for (int f = 0; f < d.O; ++f) if (tab[CEM_TASK_TAB_LO * CEM_U + f] > tab[CEM_TASK_TAB_HI * CEM_U + f]) return CEM_ERR_INVALID_ARG;
        for (int j = 0; task->rho && j < d.A; ++j) { if (!finite(task->rho[j])) return CEM_ERR_INVALID_ARG; tp.rho[j] = task->rho[j]; }
        if (!finite(task->goal_radius) || !finite(task->reward_goal) || !finite(task->reward_clip) || (bits(task->goal_radius) >> 31 && task->goal_radius != 0.f)) return CEM_ERR_INVALID_ARG;
        tp.r2 = task->goal_radius * task->goal_radius;         // fl32, rounded once here
        tp.reward_goal = task->reward_goal; tp.clip = task->reward_clip > 0.f ? task->reward_clip : inf;
    }
    if (trk) {
        if (!trk->ref || trk->ref_steps < 1 || trk->ref_steps > CEM_TASK_REF_MAX_STEPS) return CEM_ERR_INVALID_ARG;
        trk_host.assign(CEM_TASK_CLOCK_WORDS + (size_t)trk->ref_steps * CEM_U, 0u);
        for (int j = 0; j < trk->ref_steps; ++j)
            for (int f = 0; f < d.O; ++f) {
                const float v = trk->ref[(size_t)j * d.O + f];
                if (!finite(v)) return CEM_ERR_INVALID_ARG;
                trk_host[CEM_TASK_CLOCK_WORDS + (size_t)j * CEM_U + f] = bits(v);
            }
        for (int j = 0; trk->action_rate && j < d.A; ++j) { if (!finite(trk->action_rate[j])) return CEM_ERR_INVALID_ARG; kappa[j] = trk->action_rate[j]; }
    }
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.task = trk ? (int)CEM_TASK_TRACKING : on ? (int)CEM_TASK_QUADRATIC : (int)CEM_TASK_SAFETY_GYM;
    next.zones = 0;                                             // zones belong to the task they were set on (cem_planner_set_task_zones)
    next.outputs = 0;                                           // ... and so do outputs (cem_planner_set_task_outputs)
    { const int st = admit_on(h, next); if (st) return st; }
    // cem_unfold_sequences' element limit on the trajectory tensor
    const long long traj_floats = (long long)d.Bloc * (d.H + 1) * d.O;
    if (on && traj_floats > 0x7fffffff00ll) return CEM_ERR_UNSUPPORTED;
    // allocated before anything of the handle changes: a failed allocation leaves it as it was
    DevBlock made, made_trk;
    if (on && !h->task_dev) HIPCHK(made.alloc((task_tab_floats() + (size_t)traj_floats) * 4));
    if (trk) HIPCHK(made_trk.alloc(trk_host.size() * 4));         // (one per call: ref_steps is the call's)
    // Unconditional: an eager plan still draining behind its polled result may be reading the tables
    return commit_launch_change(h, next, true, [&]() -> int {
        auto drop_zones = [&] {                                 // (the stream is drained) zones and outputs alike
            if (h->zones_dev) { hipFree(h->zones_dev); h->zones_dev = nullptr; } h->zones = TaskParams{};
            if (h->outs_dev) { hipFree(h->outs_dev); h->outs_dev = nullptr; } h->outs = TaskParams{};
        };
        if (!on) { drop_zones(); return CEM_OK; }
        float *dev = made.p ? static_cast<float *>(made.p) : h->task_dev;
        if (trk) HIPCHK(hipMemcpy(made_trk.p, trk_host.data(), trk_host.size() * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(dev, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
        // (the buffer reads as zeros until the first rollout launch has filled it)
        if (made.p) HIPCHK(hipMemset(dev + task_tab_floats(), 0, (size_t)traj_floats * 4));
        if (made.p) h->task_dev = made.release<float>();
        tp.tab = h->task_dev;
        drop_zones();
        h->h_task_tab = tab;
        if (!trk) { h->task = tp; return CEM_OK; }
        // (the stream is drained: nothing reads the previous call's table or clock any more)
        if (h->track_dev) hipFree(h->track_dev);
        h->track_dev = made_trk.release<uint32_t>();
        h->track = tp;                                          // the quadratic task's fields, and the tracking task's own
        std::memcpy(h->track.kappa, kappa, sizeof kappa);
        h->track.T = trk->ref_steps; h->track.clock = h->track_dev; h->track.ref = track_ref(h->track_dev);
        h->h_clock.assign(CEM_TASK_CLOCK_WORDS, 0u);
        return CEM_OK;
    });
}

int cem_planner_set_task(cem_planner_t *h, const cem_task_t *task)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (task && task->kind != CEM_TASK_SAFETY_GYM && task->kind != CEM_TASK_QUADRATIC) return CEM_ERR_INVALID_ARG;
    return set_task(h, task, nullptr);
}

int cem_planner_set_task_tracking(cem_planner_t *h, const cem_task_t *base, const cem_task_tracking_t *trk)
{
    if (!h || !base || !trk || base->kind != CEM_TASK_QUADRATIC || base->g) return CEM_ERR_INVALID_ARG;
    return set_task(h, base, trk);
}

int cem_planner_set_task_clock(cem_planner_t *h, int32_t k0, const float *prev_action)
{
    if (!h || k0 < 0) return CEM_ERR_INVALID_ARG;
    const int A = h->d.A;
    for (int j = 0; prev_action && j < A; ++j) { uint32_t u; std::memcpy(&u, &prev_action[j], 4); if ((u & 0x7fffffffu) >= 0x7f800000u) return CEM_ERR_INVALID_ARG; }   // by its bits (-fno-honor-nans)
    if (h->opt.task != CEM_TASK_TRACKING || !h->track_dev || h->in_plan) return CEM_ERR_STATE;
    // through a copy the handle owns (as cem_planner_set_cost_budget): the caller's array need not outlive this call; no wait, the graph stays
    h->h_clock[0] = (uint32_t)k0;
    if (prev_action) std::memcpy(&h->h_clock[1], prev_action, (size_t)A * 4);
    HIPCHK(hipMemcpyAsync(h->track_dev, h->h_clock.data(), (size_t)CEM_TASK_CLOCK_WORDS * 4, hipMemcpyHostToDevice, h->stream));
    return CEM_OK;
}

// The zones of the task in force (cem_task_zones.h).  What the kernel reads besides the zone table is the base task's: a tracking task's
// own tables, reference and clock; for a quadratic task, which has no such things, a restatement of it as a tracking task inside the
// zones' own allocation
int cem_planner_set_task_zones(cem_planner_t *h, const cem_task_zones_t *zones)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    if (!zones) {
        if (h->in_plan) return CEM_ERR_STATE;
        if (!h->opt.zones) return CEM_OK;                      // nothing to clear: the handle, its graph included, stays as it is
        PlanOptions next = options_of(h); next.zones = 0;
        return commit_launch_change(h, next, true, [&]() -> int {
            if (h->zones_dev) { hipFree(h->zones_dev); h->zones_dev = nullptr; }
            h->zones = TaskParams{};
            return CEM_OK;
        });
    }
    // on the bit patterns: this file is built with -fno-honor-nans
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    auto finite = [&](float v) { return (bits(v) & 0x7fffffffu) < 0x7f800000u; };
    auto below_zero = [&](float v) { return (bits(v) >> 31) != 0u && (bits(v) & 0x7fffffffu) != 0u; };
    const int nz = zones->n_zones;
    if (nz < 1 || nz > CEM_TASK_MAX_ZONES || !zones->axis || !zones->centre || !zones->weight || !zones->radius) return CEM_ERR_INVALID_ARG;
    // the allocation as the kernel reads it; a zone from n_zones on has no axis and no penalty
    std::vector<uint32_t> host(kZoneWords, 0u);
    for (int z = 0; z < CEM_TASK_MAX_ZONES; ++z)
        for (int a = 0; a < CEM_TASK_ZONE_AXES; ++a) host[(size_t)z * CEM_TASK_ZONE_WORDS + CEM_TASK_ZONE_ROW_AXIS + a] = 0xffffffffu;
    for (int z = 0; z < nz; ++z) {
        uint32_t *const w = &host[(size_t)z * CEM_TASK_ZONE_WORDS];
        int used = 0;
        for (int a = 0; a < CEM_TASK_ZONE_AXES; ++a) {
            const int32_t ax = zones->axis[z * CEM_TASK_ZONE_AXES + a];
            if (ax < -1 || ax >= d.O + h->opt.outputs) return CEM_ERR_INVALID_ARG;    // (an output's index only while outputs are in force)
            if (ax < 0) continue;
            const float c = zones->centre[z * CEM_TASK_ZONE_AXES + a], wt = zones->weight[z * CEM_TASK_ZONE_AXES + a];
            if (!finite(c) || !finite(wt) || below_zero(wt)) return CEM_ERR_INVALID_ARG;
            w[CEM_TASK_ZONE_ROW_AXIS + a] = (uint32_t)ax; w[CEM_TASK_ZONE_ROW_CENTRE + a] = bits(c); w[CEM_TASK_ZONE_ROW_WEIGHT + a] = bits(wt);
            ++used;
        }
        if (!used) return CEM_ERR_INVALID_ARG;
        const float radius = zones->radius[z], margin = zones->margin ? zones->margin[z] : 0.f, penalty = zones->penalty ? zones->penalty[z] : 0.f;
        const int32_t keep_in = zones->keep_in ? zones->keep_in[z] : 0;
        if (!finite(radius) || !finite(margin) || !finite(penalty) || below_zero(margin) || below_zero(penalty)) return CEM_ERR_INVALID_ARG;
        if ((bits(radius) >> 31) != 0u || (bits(radius) & 0x7fffffffu) == 0u) return CEM_ERR_INVALID_ARG;                    // radius <= 0
        if (keep_in != 0 && keep_in != 1) return CEM_ERR_INVALID_ARG;
        if (keep_in && margin > radius) return CEM_ERR_INVALID_ARG;
        const float reach = keep_in ? radius - margin : radius + margin;
        const float R2 = radius * radius, Rm2 = reach * reach;                              // fl32, each rounded once here
        if (!finite(R2) || !finite(Rm2)) return CEM_ERR_INVALID_ARG;
        w[CEM_TASK_ZONE_R2] = bits(R2); w[CEM_TASK_ZONE_RM2] = bits(Rm2); w[CEM_TASK_ZONE_PENALTY] = bits(penalty); w[CEM_TASK_ZONE_KEEP_IN] = (uint32_t)keep_in;
    }
    if (!h->opt.task || !h->task_dev || h->in_plan) return CEM_ERR_STATE;
    const bool tracking = h->opt.task == CEM_TASK_TRACKING;
    if (tracking && !h->track_dev) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.zones = nz;
    { const int st = admit_on(h, next); if (st) return st; }
    const bool outs = h->opt.outputs != 0;                     // the task with its outputs is the base then, a tracking task whatever its kind
    if (outs && !h->outs_dev) return CEM_ERR_STATE;
    TaskParams zp = outs ? h->outs : tracking ? h->track : h->task;   // the base task as a whole: its tables, reference, clock and scalars
    zp.n_zones = nz;
    if (!tracking && !outs) {
        // the quadratic task as a tracking task: qT = q, one reference row g, kappa = 0 (as set_task left it), the clock at (0, zeros)
        if (h->h_task_tab.size() != task_tab_floats()) return CEM_ERR_STATE;
        zp.T = 1;
        std::memcpy(&host[kZoneTabAt], h->h_task_tab.data(), task_tab_floats() * 4);
        std::memcpy(&host[kZoneTabAt + (size_t)CEM_TASK_TAB_QT * CEM_U], &h->h_task_tab[(size_t)CEM_TASK_TAB_Q * CEM_U], (size_t)CEM_U * 4);
        std::memcpy(&host[kZoneRefAt], &h->h_task_tab[(size_t)CEM_TASK_TAB_G * CEM_U], (size_t)CEM_U * 4);
    }
    // allocated before anything of the handle changes: a failed allocation leaves it as it was
    DevBlock made;
    HIPCHK(made.alloc(kZoneWords * 4));
    // Unconditional: an eager plan still draining behind its polled result may be reading the previous zones
    return commit_launch_change(h, next, true, [&]() -> int {
        HIPCHK(hipMemcpy(made.p, host.data(), kZoneWords * 4, hipMemcpyHostToDevice));
        if (h->zones_dev) hipFree(h->zones_dev);
        h->zones_dev = made.release<uint32_t>();
        zp.zones = h->zones_dev;
        if (!tracking && !outs) {
            zp.tab = reinterpret_cast<const float *>(h->zones_dev + kZoneTabAt); zp.ref = reinterpret_cast<const float *>(h->zones_dev + kZoneRefAt);
            zp.clock = h->zones_dev + kZoneClockAt;
        }
        h->zones = zp;
        return CEM_OK;
    });
}

// The linear outputs of the task in force (cem_task_outputs.h).  The allocation holds C, the outputs' tables and reference, an empty
// zone table (the kernel is the zones kind's superset and reads one) and, for a quadratic base, its restatement as a tracking task
// exactly as cem_planner_set_task_zones makes it.  The zones are cleared: they are set on the task WITH its outputs
int cem_planner_set_task_outputs(cem_planner_t *h, const cem_task_outputs_t *outputs)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    auto drop = [](cem_planner_t *h) {
        if (h->zones_dev) { hipFree(h->zones_dev); h->zones_dev = nullptr; } h->zones = TaskParams{};
        if (h->outs_dev) { hipFree(h->outs_dev); h->outs_dev = nullptr; } h->outs = TaskParams{};
    };
    if (!outputs) {
        if (h->in_plan) return CEM_ERR_STATE;
        if (!h->opt.outputs) return CEM_OK;                    // nothing to clear: the handle, its graph and its zones included, stays as it is
        PlanOptions next = options_of(h); next.outputs = 0; next.zones = 0;
        return commit_launch_change(h, next, true, [&]() -> int { drop(h); return CEM_OK; });
    }
    // on the bit patterns: this file is built with -fno-honor-nans
    auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u; };
    auto finite = [&](float v) { return (bits(v) & 0x7fffffffu) < 0x7f800000u; };
    auto is_nan = [&](float v) { return (bits(v) & 0x7fffffffu) > 0x7f800000u; };
    auto below_zero = [&](float v) { return (bits(v) >> 31) != 0u && (bits(v) & 0x7fffffffu) != 0u; };
    const int M = outputs->n_outputs;
    if (M < 1 || M > CEM_TASK_MAX_OUTPUTS || !outputs->matrix) return CEM_ERR_INVALID_ARG;
    const int rows = outputs->reference ? outputs->ref_rows : 1;
    if (rows < 1 || rows > CEM_TASK_REF_MAX_STEPS) return CEM_ERR_INVALID_ARG;
    // the allocation as the kernel reads it; an output from n_outputs on has a zero row, zero weights and infinite bounds
    std::vector<uint32_t> host(kOutRefAt + (size_t)rows * CEM_TASK_MAX_OUTPUTS, 0u);
    const float inf = std::numeric_limits<float>::infinity();
    for (int m = 0; m < M; ++m)
        for (int f = 0; f < d.O; ++f) {
            const float v = outputs->matrix[(size_t)m * d.O + f];
            if (!finite(v)) return CEM_ERR_INVALID_ARG;
            host[(size_t)m * CEM_U + f] = bits(v);
        }
    uint32_t *const tab = &host[kOutTabAt];
    for (int m = 0; m < CEM_TASK_MAX_OUTPUTS; ++m) { tab[CEM_TASK_OUT_TAB_LO * CEM_TASK_MAX_OUTPUTS + m] = bits(-inf); tab[CEM_TASK_OUT_TAB_HI * CEM_TASK_MAX_OUTPUTS + m] = bits(inf); }
    for (int m = 0; m < M; ++m) {
        const float w = outputs->weight ? outputs->weight[m] : 0.f, g = outputs->target ? outputs->target[m] : 0.f, c = outputs->linear ? outputs->linear[m] : 0.f;
        const float nr = outputs->near ? outputs->near[m] : 0.f, lo = outputs->lo ? outputs->lo[m] : -inf, hi = outputs->hi ? outputs->hi[m] : inf;
        const float wT = outputs->terminal ? outputs->terminal[m] : w;
        if (!finite(w) || !finite(g) || !finite(c) || !finite(nr) || !finite(wT) || below_zero(w) || below_zero(wT)) return CEM_ERR_INVALID_ARG;
        if (is_nan(lo) || is_nan(hi) || lo > hi) return CEM_ERR_INVALID_ARG;
        tab[CEM_TASK_OUT_TAB_Q * CEM_TASK_MAX_OUTPUTS + m] = bits(w); tab[CEM_TASK_OUT_TAB_QT * CEM_TASK_MAX_OUTPUTS + m] = bits(wT);
        tab[CEM_TASK_OUT_TAB_C * CEM_TASK_MAX_OUTPUTS + m] = bits(c); tab[CEM_TASK_OUT_TAB_M * CEM_TASK_MAX_OUTPUTS + m] = bits(nr);
        tab[CEM_TASK_OUT_TAB_LO * CEM_TASK_MAX_OUTPUTS + m] = bits(lo); tab[CEM_TASK_OUT_TAB_HI * CEM_TASK_MAX_OUTPUTS + m] = bits(hi);
        for (int j = 0; j < rows; ++j) {
            const float v = outputs->reference ? outputs->reference[(size_t)j * M + m] : g;
            if (!finite(v)) return CEM_ERR_INVALID_ARG;
            host[kOutRefAt + (size_t)j * CEM_TASK_MAX_OUTPUTS + m] = bits(v);
        }
    }
    for (int z = 0; z < CEM_TASK_MAX_ZONES; ++z)
        for (int a = 0; a < CEM_TASK_ZONE_AXES; ++a) host[kOutZoneAt + (size_t)z * CEM_TASK_ZONE_WORDS + CEM_TASK_ZONE_ROW_AXIS + a] = 0xffffffffu;
    if (!h->opt.task || !h->task_dev || h->in_plan) return CEM_ERR_STATE;
    const bool tracking = h->opt.task == CEM_TASK_TRACKING;
    if (tracking && !h->track_dev) return CEM_ERR_STATE;
    if (rows != 1 && rows != (tracking ? h->track.T : 1)) return CEM_ERR_INVALID_ARG;
    PlanOptions next = options_of(h); next.outputs = M; next.zones = 0;
    { const int st = admit_on(h, next); if (st) return st; }
    TaskParams op = tracking ? h->track : h->task;             // the base task as a whole: its tables, reference, clock and scalars
    op.n_zones = 0; op.n_outputs = M; op.out_T = rows;
    if (!tracking) {
        // the quadratic task as a tracking task, as the zones make it: qT = q, one reference row g, kappa = 0, the clock at (0, zeros);
        // an output's terminal weight is its weight there
        if (h->h_task_tab.size() != task_tab_floats()) return CEM_ERR_STATE;
        op.T = 1;
        std::memcpy(&host[kOutZoneAt + kZoneTabAt], h->h_task_tab.data(), task_tab_floats() * 4);
        std::memcpy(&host[kOutZoneAt + kZoneTabAt + (size_t)CEM_TASK_TAB_QT * CEM_U], &h->h_task_tab[(size_t)CEM_TASK_TAB_Q * CEM_U], (size_t)CEM_U * 4);
        std::memcpy(&host[kOutZoneAt + kZoneRefAt], &h->h_task_tab[(size_t)CEM_TASK_TAB_G * CEM_U], (size_t)CEM_U * 4);
        std::memcpy(&tab[CEM_TASK_OUT_TAB_QT * CEM_TASK_MAX_OUTPUTS], &tab[CEM_TASK_OUT_TAB_Q * CEM_TASK_MAX_OUTPUTS], (size_t)CEM_TASK_MAX_OUTPUTS * 4);
    }
    // allocated before anything of the handle changes: a failed allocation leaves it as it was
    DevBlock made;
    HIPCHK(made.alloc(host.size() * 4));
    // Unconditional: an eager plan still draining behind its polled result may be reading the previous outputs or zones
    return commit_launch_change(h, next, true, [&]() -> int {
        HIPCHK(hipMemcpy(made.p, host.data(), host.size() * 4, hipMemcpyHostToDevice));
        drop(h);
        h->outs_dev = made.release<uint32_t>();
        const float *const base = reinterpret_cast<const float *>(h->outs_dev);
        op.out_c = base; op.out_tab = base + kOutTabAt; op.out_ref = base + kOutRefAt;
        op.zones = h->outs_dev + kOutZoneAt;
        if (!tracking) { op.tab = base + kOutZoneAt + kZoneTabAt; op.ref = base + kOutZoneAt + kZoneRefAt; op.clock = h->outs_dev + kOutZoneAt + kZoneClockAt; }
        h->outs = op;
        return CEM_OK;
    });
}

int cem_planner_task_trajectories(cem_planner_t *h, float *out_dev)
{
    if (!h || !out_dev) return CEM_ERR_INVALID_ARG;
    if (!h->opt.task || !h->task_dev) return CEM_ERR_STATE;
    const Dims &d = h->d;
    HIPCHK(hipMemcpyAsync(out_dev, task_traj(h), (size_t)d.Bloc * (d.H + 1) * d.O * 4, hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_task_score(cem_planner_t *h, const float *traj_dev, const float *actions_dev, int32_t n_rows, int32_t horizon,
                   float *ret_out_dev, uint8_t *costs_out_dev)
{
    if (!h || !traj_dev || !actions_dev || !ret_out_dev || n_rows < 1 || horizon < 1 || horizon > 65535) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;
    if (!h->opt.task || !h->task_dev) return CEM_ERR_STATE;
    const Dims &d = h->d;
    if (n_rows % d.P != 0) return CEM_ERR_INVALID_ARG;                 // reshape(cum, (particles, -1)) would raise (mpc_policy.py:38)
    if ((long long)n_rows * (horizon + 1) * d.O > 0x7fffffff00ll) return CEM_ERR_UNSUPPORTED;
    TaskParams io{};                                            // (a tracking task: with the handle's clock, as a plan)
    io.traj = traj_dev; io.actions = actions_dev; io.ctrl = nullptr; io.ret = ret_out_dev;
    io.costs = h->cfg.variant != CEM_VARIANT_CEM ? costs_out_dev : nullptr;
    io.rows = n_rows; io.N = n_rows / d.P; io.H = horizon; io.check_done = 0;
    { const int st = task_launch(h, io, CEM_ERR_STATE); if (st) return st; }
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_planner_get_elite_carry(const cem_planner_t *h, cem_elite_carry_t *out)
{
    if (!h || !out) return CEM_ERR_INVALID_ARG;
    *out = h->opt.elite;
    return CEM_OK;
}

int cem_planner_elite_store(cem_planner_t *h, int32_t problem, float *out_host, int32_t *count_out)
{
    if (!h || problem < 0 || problem >= warm_slots(h) || (!out_host && !count_out)) return CEM_ERR_INVALID_ARG;
    if (!h->opt.elite.n_keep || !h->elite_dev) return CEM_ERR_STATE;
    HIPCHK(hipStreamSynchronize(h->stream));
    const size_t row = (size_t)h->opt.elite.n_keep * h->d.H * h->d.A;
    if (out_host) HIPCHK(hipMemcpy(out_host, elite_store(h) + (size_t)problem * row, row * 4, hipMemcpyDeviceToHost));
    if (count_out) HIPCHK(hipMemcpy(count_out, elite_counts(h) + problem, 4, hipMemcpyDeviceToHost));
    return CEM_OK;
}

int cem_planner_set_population_schedule(cem_planner_t *h, const int32_t *n, int32_t count)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    const Dims &d = h->d;
    if (count != 0 && count != d.I) return CEM_ERR_INVALID_ARG;
    if (!n) count = 0;
    bool on = false;
    for (int it = 0; it < count; ++it) {
        if (n[it] < d.k || n[it] > d.N || ((long long)d.P * n[it]) % d.E != 0) return CEM_ERR_INVALID_ARG;
        on = on || n[it] != d.N;
    }
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.pop.clear();
    if (on) next.pop.assign(n, n + count);
    // (every population's select mode is asked here, in front of the per-iteration validate below, where it used to be asked behind it:
    // the arguments above leave validate nothing to refuse on a one-rank handle, and a smaller population never leaves the one-workgroup select)
    { const int st = admit_on(h, next); if (st) return st; }
    std::vector<IterPlan> plans;
    std::vector<std::vector<Tile6>> lists;
    DevBlock block; uint32_t *flags = (uint32_t *)(h->ws + h->lay.seg_flags); f4 *state = (f4 *)(h->ws + h->lay.seg_state);
    size_t n_ready = 0, flags_off = 0, flags_bytes = 0, state_bytes = 0;
    if (on) {
        // every iteration's plan, from the functions create uses, for the configuration that differs in n_samples alone
        plans.resize(d.I); lists.resize(d.I);
        size_t bytes = 0;
        for (int it = 0; it < d.I; ++it) {
            IterPlan &ip = plans[it];
            if (n[it] == d.N) {
                ip.d = h->d; ip.rc = h->rc; ip.n_tiles = h->n_tiles; ip.n_seg = h->n_seg; ip.seg_len = h->seg_len; ip.n_pinned = h->n_pinned;
                ip.sample_in_rollout = h->sample_in_rollout; ip.lean_rollout = h->lean_rollout; ip.tiles_off = (size_t)-1;
            } else {
                cem_config_t c = h->cfg; c.n_samples = n[it];
                { const int st = validate(&c); if (st) return st; }
                ip.d = make_dims(&c);
                const Plan pl = make_plan(&c, ip.d);
                ip.rc = pl.rc; ip.n_seg = pl.n_seg; ip.seg_len = pl.seg_len; ip.n_pinned = pl.n_pinned;
                build_plan_tiles(ip.d, ip.rc, lists[it]);
                ip.n_tiles = (int)lists[it].size();
                place_sampler(h, ip.d, pl, &ip.sample_in_rollout, &ip.lean_rollout);
                ip.tiles_off = bytes; bytes += align256(lists[it].size() * sizeof(Tile6));
            }
            if (ip.n_seg > 1) {
                const size_t n_float = (size_t)(ip.n_tiles - ip.n_pinned);
                n_ready = std::max(n_ready, n_float * (ip.n_seg - 1));
                state_bytes = std::max(state_bytes, n_float * (2 * (size_t)ip.d.NFW * ip.rc * 256 + 64) * 16);
            }
        }
        flags_bytes = n_ready * 4;
        // the workspace's two arrays serve while they are large enough (their sizes: up to the next array's offset); else both move
        const bool own_seg = flags_bytes > h->lay.seg_state - h->lay.seg_flags || state_bytes > h->lay.ms_hist - h->lay.seg_state;
        if (own_seg) { flags_off = bytes; bytes += align256(flags_bytes) + align256(state_bytes); }
        // allocated and filled before anything of the handle changes: a failed call leaves it as it was
        HIPCHK(block.alloc(std::max<size_t>(bytes, 256)));
        char *base = (char *)block.p;
        for (int it = 0; it < d.I; ++it)
            if (plans[it].tiles_off != (size_t)-1)
                HIPCHK(hipMemcpy(base + plans[it].tiles_off, lists[it].data(), lists[it].size() * sizeof(Tile6), hipMemcpyHostToDevice));
        if (own_seg) {
            HIPCHK(hipMemset(base + flags_off, 0, align256(flags_bytes) + align256(state_bytes)));
            flags = (uint32_t *)(base + flags_off); state = (f4 *)(base + flags_off + align256(flags_bytes));
        }
    }
    // Unconditional, as in cem_planner_set_elite_carry: an eager plan still draining behind its polled result may be reading the old lists
    return commit_launch_change(h, next, true, [&]() -> int {
        if (h->pop_dev) hipFree(h->pop_dev);
        h->pop_dev = block.release<char>(); h->pop.swap(plans); h->pop_seg_flags = flags; h->pop_seg_state = state; h->pop_n_ready = (int)n_ready;
        return CEM_OK;
    });
}

int cem_planner_get_population_schedule(const cem_planner_t *h, int32_t *n_out, int32_t count, int32_t *enabled_out)
{
    if (!h || (!n_out && !enabled_out) || (n_out && count != h->d.I)) return CEM_ERR_INVALID_ARG;
    if (n_out) for (int it = 0; it < h->d.I; ++it) n_out[it] = iter_view(h, it).d->N;
    if (enabled_out) *enabled_out = h->pop.empty() ? 0 : 1;
    return CEM_OK;
}

int cem_planner_set_mean_candidate(cem_planner_t *h, int32_t enable)
{
    if (!h || (enable != 0 && enable != 1)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.mean_cand = enable;
    { const int st = admit_on(h, next); if (st) return st; }
    return commit_launch_change(h, next, false);
}

int cem_planner_get_mean_candidate(const cem_planner_t *h, int32_t *enable_out)
{
    if (!h || !enable_out) return CEM_ERR_INVALID_ARG;
    *enable_out = h->opt.mean_cand;
    return CEM_OK;
}

int cem_planner_set_initial_distribution(cem_planner_t *h, int32_t slot, const float *mu, const float *sigma)
{
    if (!h || !mu || !sigma || slot < 0 || slot >= warm_slots(h)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    const size_t HA = (size_t)h->d.H * h->d.A;
    for (size_t i = 0; i < HA; ++i) if (!finite_bits(mu[i]) || !finite_bits(sigma[i]) || sigma[i] < 0.f) return CEM_ERR_INVALID_ARG;
    // through a copy the handle owns: a previous plan may still be draining behind its polled result, and the caller's arrays need
    // not outlive this call
    float *dst = h->h_expl.data() + (size_t)slot * 2 * HA;
    std::memcpy(dst, mu, HA * 4); std::memcpy(dst + HA, sigma, HA * 4);
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.expl + (size_t)slot * 2 * HA * 4, dst, 2 * HA * 4, hipMemcpyHostToDevice, h->stream));
    h->have_expl[slot] = 1;
    return CEM_OK;
}

int cem_planner_set_init_mode(cem_planner_t *h, int32_t slot, int32_t mode)
{
    if (!h || slot < -1 || slot >= warm_slots(h)) return CEM_ERR_INVALID_ARG;
    if (mode != CEM_INIT_COLD && mode != CEM_INIT_EXPLICIT && mode != CEM_INIT_SHIFT) return CEM_ERR_INVALID_ARG;
    for (int s = 0; s < warm_slots(h); ++s) if (slot < 0 || s == slot) h->slot_mode[s] = mode;
    return CEM_OK;
}

int cem_planner_reset_carry(cem_planner_t *h, int32_t slot)
{
    if (!h || slot < -1 || slot >= warm_slots(h)) return CEM_ERR_INVALID_ARG;
    for (int s = 0; s < warm_slots(h); ++s) if (slot < 0 || s == slot) { h->carry_valid[s] = 0; h->carry_at[s] = -1; }
    // the kept elites of the slot(s) go with it (cem_elite_carry.h): stream-ordered, so a plan still draining finishes with what it had
    if (h->elite_dev) HIPCHK(hipMemsetAsync(elite_counts(h) + (slot < 0 ? 0 : slot), 0, (size_t)(slot < 0 ? warm_slots(h) : 1) * 4, h->stream));
    return CEM_OK;
}

int cem_planner_get_carry(cem_planner_t *h, int32_t slot, float *mu, float *sigma, int32_t *valid)
{
    if (!h || slot < 0 || slot >= warm_slots(h)) return CEM_ERR_INVALID_ARG;
    const size_t HA = (size_t)h->d.H * h->d.A;
    if (h->in_plan) return CEM_ERR_STATE;               // a stepwise plan is open: the slot's slice holds that plan's distribution
    const bool ok = h->carry_valid[slot] != 0;
    if (valid) *valid = ok ? 1 : 0;
    if (!ok) {
        if (mu) std::memset(mu, 0, HA * 4);
        if (sigma) std::memset(sigma, 0, HA * 4);
        return CEM_OK;
    }
    // where the carry is right now: still in the mu / sigma slice of the problem that ran it, or already moved to the slot's buffer
    const char *src = h->carry_at[slot] >= 0 ? h->ws + h->lay.musig + (size_t)h->carry_at[slot] * 2 * HA * 4 : h->ws + h->lay.carry + (size_t)slot * 2 * HA * 4;
    if (mu) HIPCHK(hipMemcpyAsync(mu, src, HA * 4, hipMemcpyDeviceToHost, h->stream));
    if (sigma) HIPCHK(hipMemcpyAsync(sigma, src + HA * 4, HA * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_planner_set_carry_slots(cem_planner_t *h, int32_t n, const int32_t *slots)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (!h->batch) return CEM_ERR_STATE;
    if (n < 1 || n > h->batch) return CEM_ERR_INVALID_ARG;
    std::vector<int32_t> map(h->batch); std::vector<uint8_t> used(h->batch, 0);
    for (int b = 0; b < n; ++b) {
        const int32_t s = slots ? slots[b] : b;
        if (s < 0 || s >= h->batch || used[s]) return CEM_ERR_INVALID_ARG;
        used[s] = 1; map[b] = s;
    }
    for (int b = n, s = 0; b < h->batch; ++b) { while (used[s]) ++s; used[s] = 1; map[b] = s; }   // the rest, ascending: always a permutation
    h->slot_of.swap(map);
    return CEM_OK;
}

int cem_comm_unique_id(void *id_out)
{
    if (!id_out) return CEM_ERR_INVALID_ARG;
    Rccl *r = rccl(); if (!r) return CEM_ERR_COMM;
    CemNcclId id;
    NCCLCHK(r->GetUniqueId(&id));
    std::memcpy(id_out, id.internal, CEM_COMM_ID_BYTES);
    return CEM_OK;
}

int cem_planner_comm_init(cem_planner_t *h, const void *id, int32_t n_ranks, int32_t rank)
{
    if (!h || !id) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;                                        // batch handles are single-rank
    if (n_ranks != h->d.W || rank != h->d.R) return CEM_ERR_INVALID_ARG;       // the communicator IS the candidate sharding of this handle
    if (h->in_plan) return CEM_ERR_STATE;
    PlanOptions next = options_of(h); next.comm = true;
    { const int st = admit_on(h, next); if (st) return st; }
    Rccl *r = rccl(); if (!r) return CEM_ERR_COMM;
    if (h->comm) { r->CommDestroy(h->comm); h->comm = nullptr; }
    CemNcclId nid; std::memcpy(nid.internal, id, CEM_COMM_ID_BYTES);
    void *comm = nullptr;
    NCCLCHK(r->CommInitRank(&comm, n_ranks, nid, rank));
    h->comm = comm; h->plans_since_comm = 0;
    // a graph captured without the collective (world 1) no longer describes the plan
    drop_graph(h); h->graph_failed = false;
    return CEM_OK;
}

int cem_planner_comm_ranks(const cem_planner_t *h, int32_t *n_ranks_out)
{
    if (!h || !n_ranks_out) return CEM_ERR_INVALID_ARG;
    *n_ranks_out = 0;
    if (!h->comm) return CEM_OK;                     // no communicator: 0
    Rccl *r = rccl(); if (!r || !r->CommCount) return CEM_ERR_COMM;
    int n = 0;
    NCCLCHK(r->CommCount(h->comm, &n));
    *n_ranks_out = n;
    return CEM_OK;
}

int cem_planner_comm_destroy(cem_planner_t *h)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    if (h->comm) {
        HIPCHK(hipStreamSynchronize(h->stream));
        if (Rccl *r = rccl()) r->CommDestroy(h->comm);
        h->comm = nullptr;
        drop_graph(h);
    }
    return CEM_OK;
}

int cem_planner_graph_status(const cem_planner_t *h, int32_t *status_out)
{
    if (!h || !status_out) return CEM_ERR_INVALID_ARG;
    *status_out = h->graph_ready ? 1 : (h->graph_failed ? 2 : 0);
    return CEM_OK;
}

int cem_planner_graph_nodes(const cem_planner_t *h, int32_t *nodes_out)
{
    if (!h || !nodes_out) return CEM_ERR_INVALID_ARG;
    size_t n = 0;
    if (h->graph_ready && h->graph) HIPCHK(hipGraphGetNodes(h->graph, nullptr, &n));
    *nodes_out = (int32_t)n;
    return CEM_OK;
}

int cem_planner_rollout_path(const cem_planner_t *h, int32_t *path_out)
{
    if (!h || !path_out) return CEM_ERR_INVALID_ARG;
    *path_out = recipe_of(h, 0, false).lean_form ? 1 : 0;
    return CEM_OK;
}

int cem_planner_rollout_form(const cem_planner_t *h, int32_t it, int32_t *form_out)
{
    if (!h || !form_out || it < 0 || it >= h->d.I) return CEM_ERR_INVALID_ARG;
    *form_out = recipe_of(h, it, false).lean_form;
    return CEM_OK;
}

int cem_planner_launches_per_iteration(const cem_planner_t *h, int32_t *launches_out)
{
    if (!h || !launches_out) return CEM_ERR_INVALID_ARG;
    *launches_out = launches_of(h, 0);
    return CEM_OK;
}

int cem_planner_iteration_plan(const cem_planner_t *h, int32_t it, cem_iteration_plan_t *out)
{
    if (!h || !out || it < 0 || it >= h->d.I) return CEM_ERR_INVALID_ARG;
    const IterView v = iter_view(h, it);
    out->n_samples = v.d->N; out->chunks_per_tile = v.rc; out->n_tiles = v.n_tiles; out->n_segments = v.n_seg; out->n_pinned = v.n_pinned;
    out->launches = launches_of(h, it);
    out->rollout_path = recipe_of(h, it, false).lean_form ? 1 : 0;
    out->reserved = 0;
    return CEM_OK;
}

int cem_plan_exchange(cem_planner_t *h)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (!h->in_plan || !h->comm) return CEM_ERR_STATE;
    return enqueue_exchange(h);
}

// grow-only device scratch of the standalone ops, cached on the handle (a hipMalloc / hipFree pair per call is a
// device-wide synchronisation each)
static int ensure_scratch(cem_planner *h, size_t bytes)
{
    if (bytes <= h->scratch_bytes) return CEM_OK;
    if (h->scratch) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipFree(h->scratch)); h->scratch = nullptr; h->scratch_bytes = 0; }
    const size_t want = align256(bytes + bytes / 2);
    HIPCHK(hipMalloc((void **)&h->scratch, want));
    h->scratch_bytes = want;
    return CEM_OK;
}

// Philox key of a standalone call: only the 16-byte (seed, call) prefix of the device control block is written, and never
// while a stepwise plan is in flight (its best-so-far / early-stop state and its own key live in the same block)
static int upload_key(cem_planner *h, uint64_t seed, uint64_t call)
{
    CtrlBlock *c = h->h_ctrl;
    c->seed_lo = (uint32_t)seed; c->seed_hi = (uint32_t)(seed >> 32); c->call_lo = (uint32_t)call; c->call_hi = (uint32_t)(call >> 32);
    HIPCHK(hipMemcpyAsync(h->ws + h->lay.ctrl, c, 16, hipMemcpyHostToDevice, h->stream));
    return CEM_OK;
}

int cem_unfold_sequences(cem_planner_t *h, const float *s0_dev, const float *actions_dev, int32_t n_rows, int32_t horizon,
                         const float *eps_model_dev, uint64_t seed, uint64_t call, float *traj_out_dev, float *mu_out_dev, float *sd_out_dev)
{
    if (!h || !s0_dev || !actions_dev || n_rows < 1 || horizon < 1 || horizon > 65535) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;                  // the model ops run on single-state handles
    if (!h->have_weights) return CEM_ERR_NO_WEIGHTS;
    if (h->in_plan) return CEM_ERR_STATE;
    const Dims &d = h->d;
    if (n_rows % d.E != 0) return CEM_ERR_SPLIT;
    if ((long long)n_rows * (horizon + 1) * d.O > 0x7fffffff00ll) return CEM_ERR_UNSUPPORTED;
    const int chunk = n_rows / d.E;
    const int rc = d.wide ? 1 : (d.split() ? (n_rows >= 256 * 32 ? 2 : 1) : (n_rows >= 256 * 64 ? 4 : (n_rows >= 256 * 32 ? 2 : 1)));
    std::vector<Tile6> tiles;
    for (int m = 0; m < d.E; ++m)
        for (int r = m * chunk; r < (m + 1) * chunk; r += 16 * rc) {
            Tile6 t; t.v[0] = r; t.v[1] = std::min(16 * rc, (m + 1) * chunk - r); t.v[2] = m; t.v[3] = r; t.v[4] = r; t.v[5] = r;
            tiles.push_back(t);
        }
    const size_t tile_bytes = align256(tiles.size() * sizeof(Tile6));
    int st = ensure_scratch(h, tile_bytes + (size_t)n_rows * 4); if (st) return st;
    TileDesc *dt = (TileDesc *)h->scratch; float *ret = (float *)(h->scratch + tile_bytes);
    // the tile list is pageable host memory: the copy has returned from it when hipMemcpyAsync returns only if it was staged;
    // synchronise before `tiles` goes out of scope (below, with the kernel)
    HIPCHK(hipMemcpyAsync(dt, tiles.data(), tiles.size() * sizeof(Tile6), hipMemcpyHostToDevice, h->stream));
    st = upload_key(h, seed, call); if (st) return st;
    RolloutParams rp; fill_rollout_common(h, rp);
    rp.tiles = dt; rp.s0 = s0_dev; rp.actions = actions_dev; rp.eps_model = eps_model_dev; rp.ret = ret; rp.costs = nullptr;
    rp.traj = traj_out_dev; rp.mu_out = mu_out_dev; rp.sd_out = sd_out_dev;
    rp.H = horizon; rp.Bloc = n_rows; rp.Btot = n_rows; rp.it = 0; rp.variant = 0; rp.check_done = 0;
    hipError_t e = d.wide ? launch_rollout_wide(h, rp, (int)tiles.size(), 1)
                 : d.chunked() ? launch_rollout_chunked(d, rc, 1, rp, (int)tiles.size(), h->stream)
                               : launch_rollout<1>(rc, d.NFW, rp, (int)tiles.size(), h->stream);
    hipError_t e2 = hipStreamSynchronize(h->stream);
    HIPCHK(e); HIPCHK(e2);
    return CEM_OK;
}

int cem_compute_objective(cem_planner_t *h, const float *traj_dev, int32_t n_rows, int32_t horizon, float *scores_out_dev)
{
    if (!h || !traj_dev || !scores_out_dev || n_rows < 1 || horizon < 1 || horizon > 65535) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;
    const Dims &d = h->d;
    if (n_rows % d.P != 0) return CEM_ERR_INVALID_ARG;                 // reshape(cum, (particles, -1)) would raise (mpc_policy.py:38)
    if ((long long)n_rows * horizon > 0x7fffffffll) return CEM_ERR_UNSUPPORTED;
    const bool cost_obj = h->cfg.variant == CEM_VARIANT_COST;             // compute_mean_costs (safe_cem_mpc.py:98-108): scores = -mean cost
    const bool safe = h->cfg.variant == CEM_VARIANT_SAFE || cost_obj;     // (the safe variant's cost bytes, un-masked by sc_roll's threshold)
    if (h->opt.cost_m && (long long)horizon * h->opt.cost_m * CEM_MAX_COST_KINDS >= kBudgetTotalLimit) return CEM_ERR_UNSUPPORTED;   // (the encoding of infeasible scores)
    const size_t ret_bytes = align256((size_t)n_rows * 4);
    int st = ensure_scratch(h, ret_bytes + (safe ? (size_t)n_rows * horizon : 0)); if (st) return st;
    ObjectiveParams op{}; op.traj = traj_dev; op.ret = (float *)h->scratch; op.costs = safe ? (uint8_t *)(h->scratch + ret_bytes) : nullptr;
    op.B = n_rows; op.H = horizon; op.O = d.O; op.variant = safe ? (int)CEM_VARIANT_SAFE : h->cfg.variant; op.sc = h->sc_roll;
    hipLaunchKernelGGL(cem_objective_kernel, dim3((unsigned)(((size_t)n_rows * 16 + 255) / 256)), dim3(256), 0, h->stream, op);
    HIPCHK(hipGetLastError());
    const int n_cand = n_rows / d.P;
    if (h->opt.cost_m && (size_t)n_cand > h->cstat_obj_n) {
        if (h->cstat_obj) { HIPCHK(hipStreamSynchronize(h->stream)); HIPCHK(hipFree(h->cstat_obj)); h->cstat_obj = nullptr; h->cstat_obj_n = 0; if (h->last_cstat_problems == 0) h->last_cstat = nullptr; }
        const size_t want = (size_t)n_cand + (size_t)n_cand / 2;
        HIPCHK(hipMalloc((void **)&h->cstat_obj, want * 4));
        h->cstat_obj_n = want;
    }
    const ReduceParams sp = fill_score(h, op.ret, op.costs, scores_out_dev, h->opt.cost_m ? h->cstat_obj : nullptr, n_cand, horizon, 0, false);
    HIPCHK(launch_score(h, sp, 1));
    HIPCHK(hipStreamSynchronize(h->stream));
    if (h->opt.cost_m) { h->last_cstat = sp.cstat; h->last_cstat_n = n_cand; h->last_cstat_problems = 0; }      // (0: the op's own array)
    return CEM_OK;
}

static int scorer_op(cem_planner *h, const float *obs, const float *next_obs, int32_t n, float *out, uint8_t *flag, int what)
{
    ScorerOpParams sp{}; sp.obs = obs; sp.next_obs = next_obs; sp.out = out; sp.flag = flag; sp.n = n; sp.O = h->d.O; sp.what = what; sp.sc = h->sc;
    hipLaunchKernelGGL(cem_scorer_kernel, dim3((unsigned)(((size_t)n * 16 + 255) / 256)), dim3(256), 0, h->stream, sp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_scorer_reward(cem_planner_t *h, const float *obs_dev, const float *next_obs_dev, int32_t n, float *reward_out_dev,
                      uint8_t *goal_achieved_out_dev)
{
    if (!h || !obs_dev || !next_obs_dev || !reward_out_dev || n < 1) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;
    return scorer_op(h, obs_dev, next_obs_dev, n, reward_out_dev, goal_achieved_out_dev, 0);
}

int cem_scorer_cost(cem_planner_t *h, const float *obs_dev, int32_t n, float *cost_out_dev)
{
    if (!h || !obs_dev || !cost_out_dev || n < 1) return CEM_ERR_INVALID_ARG;
    if (h->batch) return CEM_ERR_STATE;
    return scorer_op(h, obs_dev, nullptr, n, cost_out_dev, nullptr, 1);
}

int cem_fill_noise(cem_planner_t *h, uint64_t seed, uint64_t call, float *eps_act_dev, float *eps_model_dev, float *eps_out_dev)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    const Dims &d = h->d;
    int st = upload_key(h, seed, call); if (st) return st;
    FillParams fp{}; fp.eps_act = eps_act_dev; fp.eps_model = eps_model_dev; fp.eps_out = eps_out_dev;
    fp.ctrl = (const CtrlBlock *)(h->ws + h->lay.ctrl); fp.I = d.I; fp.N = d.N; fp.H = d.H; fp.A = d.A; fp.B = d.Btot; fp.O = d.O;
    hipLaunchKernelGGL(cem_fill_noise_kernel, dim3(2048), dim3(256), 0, h->stream, fp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_philox_words(cem_planner_t *h, uint64_t seed, uint64_t call, uint32_t stream, uint32_t iteration, uint32_t t, uint32_t sub,
                     uint32_t idx0, uint32_t n, uint32_t *words_out_dev)
{
    if (!h || !words_out_dev || stream > 2 || iteration > 65535 || t > 65535 || sub > 65535) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    if (n == 0) return CEM_OK;
    int st = upload_key(h, seed, call); if (st) return st;
    WordsParams wp{}; wp.out = words_out_dev; wp.ctrl = (const CtrlBlock *)(h->ws + h->lay.ctrl);
    wp.stream = stream; wp.it = iteration; wp.t = t; wp.sub = sub; wp.idx0 = idx0; wp.n = n;
    hipLaunchKernelGGL(cem_philox_words_kernel, dim3((n + 255) / 256), dim3(256), 0, h->stream, wp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    return CEM_OK;
}

int cem_planner_select_mode(const cem_planner_t *h, int32_t *mode_out)
{
    if (!h || !mode_out) return CEM_ERR_INVALID_ARG;
    *mode_out = select_mode_now(h);
    return CEM_OK;
}

int cem_planner_select_form(const cem_planner_t *h, int32_t it, int32_t *form_out)
{
    if (!h || !form_out || it < 0 || it >= h->d.I) return CEM_ERR_INVALID_ARG;
    *form_out = recipe_of(h, it, false).select_form;
    return CEM_OK;
}

int cem_select_form_for(int32_t select_mode, int64_t n_samples, int64_t n_elite, int64_t horizon_x_act_dim, int32_t variant, int32_t *form_out)
{
    if (!form_out || select_mode < 0 || select_mode > 3 || n_samples < 1 || n_elite < 1 || n_elite > n_samples || horizon_x_act_dim < 1) return CEM_ERR_INVALID_ARG;
    bool cache = false;
    const int mode = resolve_select_mode(select_mode, n_samples, n_elite, horizon_x_act_dim, 140 * 1024, true, &cache);
    *form_out = select_ranked_form(mode, cache, n_samples, variant == CEM_VARIANT_CEM);
    return CEM_OK;
}

int cem_planner_inject_fault(cem_planner_t *h, int32_t kind)
{
    if (!h || (kind != 1 && kind != 2)) return CEM_ERR_INVALID_ARG;
    if (h->in_plan) return CEM_ERR_STATE;
    if (kind == 2) { h->inject_capture_fail = true; return CEM_OK; }      // the next capture counts as refused: eager launches for good
    h->inject_next = 1u;            // staged with the next plan's control block (stage_ctrl) and consumed by it
    return CEM_OK;
}

int cem_planner_set_timing(cem_planner_t *h, int32_t enable)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    h->timing = enable != 0;
    return CEM_OK;
}

int cem_planner_last_timing(cem_planner_t *h, float *rollout_ms_total, int32_t *rollout_launches, float *select_ms_total)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (rollout_ms_total) *rollout_ms_total = h->roll_ms;
    if (rollout_launches) *rollout_launches = h->roll_n;
    if (select_ms_total) *select_ms_total = h->sel_ms;
    return CEM_OK;
}

int cem_planner_last_timing_detail(cem_planner_t *h, float *reduce_ms_total, float *sampler_ms_total)
{
    if (!h) return CEM_ERR_INVALID_ARG;
    if (reduce_ms_total) *reduce_ms_total = h->red_ms;
    if (sampler_ms_total) *sampler_ms_total = h->samp_ms;
    return CEM_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// training
// ---------------------------------------------------------------------------------------------------------
struct cem_trainer {
    cem_train_config_t cfg;
    char *ws; hipStream_t stream; bool own_stream;
    size_t nat, scratch_pm;
    size_t oW, oM, oV, oG, oS, oL, oP, oT, total;
    bool tile_kernel;
    uint32_t steps_done;                     // training steps since create: the step index of the Dropout masks
    float *eval_part; size_t eval_part_floats;     // per-chunk loss partials of a one-launch validation pass (grown on demand, kept)
};

static_assert(CEM_TBMAX == CEM_TRAIN_MAX_BATCH, "cem_train.h and cem_mpc.h agree on the largest minibatch");

namespace {
// on the bit pattern: this file is built with -fno-honor-nans, which lets the compiler fold a NaN test on the value away
bool finite_positive(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u > 0u && u < 0x7f800000u; }                  // 0 < v < inf
bool unit_fraction(float v) { uint32_t u; std::memcpy(&u, &v, 4); return u < 0x3f800000u || u == 0x80000000u; }           // 0 <= v < 1
int validate_train(const cem_train_config_t *c)
{
    if (!c || c->abi_version != CEM_ABI_VERSION) return CEM_ERR_INVALID_ARG;
    if (c->inputs_dim < 1 || c->outputs_dim < 1 || c->n_layers < 1 || c->ensemble_size < 1 || c->batch_size < 1) return CEM_ERR_INVALID_ARG;
    if (c->units < 1 || c->activation < CEM_ACT_RELU || c->activation > CEM_ACT_GELU) return CEM_ERR_INVALID_ARG;
    if (!(c->dropout_rate >= 0.f && c->dropout_rate < 1.f)) return CEM_ERR_INVALID_ARG;
    // Adam's constants: a clipvalue of 0 (or below, or NaN) would zero or flip every gradient, an epsilon of 0 divides by sqrt(v) = 0
    if (!finite_positive(c->clipvalue) || !finite_positive(c->epsilon) || !unit_fraction(c->beta1) || !unit_fraction(c->beta2)) return CEM_ERR_INVALID_ARG;
    if (c->units > CEM_TWIDE || c->inputs_dim > CEM_U || c->outputs_dim > CEM_U || c->batch_size > CEM_TBMAX) return CEM_ERR_UNSUPPORTED;
    return CEM_OK;
}
size_t train_nat(const cem_train_config_t *c)
{
    return (size_t)c->inputs_dim * c->units + c->units + (size_t)(c->n_layers - 1) * ((size_t)c->units * c->units + c->units) +
           2 * ((size_t)c->units * c->outputs_dim + c->outputs_dim);
}
// row parts of a step of bt rows per member (TrainParams::nparts): one per 16 rows up to CEM_TPMAX; beyond, several passes per part
int train_parts(int bt) { return std::min((bt + CEM_TROWS - 1) / CEM_TROWS, CEM_TPMAX); }
// the partial-gradient, scratch and loss-partial slots the workspace holds: the most parts a step of at most batch_size rows takes,
// and never fewer than the four of a <= 64-row minibatch (the layout of every such configuration is the one it always had)
int train_parts_alloc(const cem_train_config_t &c) { return std::max(CEM_TPARTS, train_parts(c.batch_size)); }
// validation_step walks the set in chunks of batch_size rows, 64 for a larger batch_size: the validation loss does not depend on it
int eval_chunk_rows(const cem_train_config_t &c) { return std::min(c.batch_size, CEM_TB); }
void train_layout(cem_trainer *t)
{
    const cem_train_config_t &c = t->cfg;
    const int P = train_parts_alloc(c);
    t->nat = train_nat(&c);
    // per (member, row part) workgroup: the input, L hidden outputs, seven head / loss / gradient matrices — and, for swish / gelu, the L kept
    // pre-activations the backward gate of a non-monotone activation needs (cem_train.h: GemmEpi::outz)
    t->scratch_pm = (size_t)(c.n_layers + 8 + (CEM_ACT_NEEDS_Z(c.activation) ? c.n_layers : 0)) * CEM_TROWS * (c.units > CEM_TS ? CEM_TWIDE : CEM_TS);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align256(o + bytes); return r; };
    t->oW = take(t->nat * c.ensemble_size * 4); t->oM = take(t->nat * c.ensemble_size * 4); t->oV = take(t->nat * c.ensemble_size * 4);
    t->oG = take(((t->nat * c.ensemble_size + 3) & ~(size_t)3) * P * 4); t->oS = take(t->scratch_pm * c.ensemble_size * P * 4);
    t->oL = take((size_t)c.ensemble_size * 4); t->oP = take((size_t)c.ensemble_size * P * 2 * 4);
    t->oT = take(32 * sizeof(long long));            // phase stamps of -DCEM_STAMPS diagnostic builds: the LAST 256 B of the workspace
    t->total = o;
}
// the training step: the tile kernel (cem_train_tile.h; one instantiation per layer count up to CEM_TT_MAXL), otherwise the
// GEMM-by-GEMM kernel (cem_train.h), which takes any depth
template <int L>
hipError_t tile_kernel_lds(size_t lds)
{
    if (lds <= 48 * 1024) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_train_tile_kernel<L, false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void *>(&cem_train_tile_kernel<L, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
}

void launch_train_step(const cem_trainer *t, const TrainParams &p)
{
    const size_t lds = (size_t)(t->cfg.n_layers + 5) * CEM_TT_NB * CEM_TT_BLK;
    const dim3 grid(t->cfg.ensemble_size * p.nparts, t->tile_kernel ? (p.Bt + p.chunk - 1) / p.chunk : 1);
    const bool multi = p.chunk > CEM_TROWS * p.nparts;       // some part takes more than one 16-row pass
    if (!t->tile_kernel) {
        if (multi) hipLaunchKernelGGL(cem_train_step_kernel<true>, grid, dim3(CEM_TNT), 0, t->stream, p);
        else hipLaunchKernelGGL(cem_train_step_kernel<false>, grid, dim3(CEM_TNT), 0, t->stream, p);
        return;
    }
    switch (t->cfg.n_layers) {
#define CEM_CASE(LL) case LL: if (multi) hipLaunchKernelGGL((cem_train_tile_kernel<LL, true>), grid, dim3(64 * CEM_TT_WAVES), lds, t->stream, p); \
                              else hipLaunchKernelGGL((cem_train_tile_kernel<LL, false>), grid, dim3(64 * CEM_TT_WAVES), lds, t->stream, p); break;
    CEM_CASE(1) CEM_CASE(2) CEM_CASE(3) CEM_CASE(4) CEM_CASE(5) CEM_CASE(6)
#undef CEM_CASE
    }
}

void fill_train_params(const cem_trainer *t, TrainParams &p)
{
    const cem_train_config_t &c = t->cfg;
    std::memset(&p, 0, sizeof(p));
    p.W = (float *)(t->ws + t->oW); p.Mo = (float *)(t->ws + t->oM); p.Vo = (float *)(t->ws + t->oV);
    p.grad = (float *)(t->ws + t->oG); p.scratch = (float *)(t->ws + t->oS); p.loss_part = (float *)(t->ws + t->oP);
    p.D = c.inputs_dim; p.O = c.outputs_dim; p.U = c.units; p.L = c.n_layers; p.E = c.ensemble_size;
    p.nat = (uint32_t)t->nat; p.scratch_per_member = (uint32_t)t->scratch_pm;
    p.gpart = (uint32_t)((t->nat * c.ensemble_size + 3) & ~(size_t)3);
    p.ts = c.units > CEM_TS ? CEM_TWIDE : CEM_TS;
    p.beta1 = c.beta1; p.beta2 = c.beta2; p.eps = c.epsilon; p.clip = c.clipvalue; p.act = c.activation;
    if (c.dropout_rate > 0.f) {
        p.drop_thresh = (uint32_t)std::min(4294967295.0, std::floor((double)c.dropout_rate * 4294967296.0));
        p.drop_keep = 1.0f - c.dropout_rate; p.drop_scale = 1.0f / p.drop_keep;
        p.drop_k0 = c.dropout_seed_lo; p.drop_k1 = c.dropout_seed_hi; p.drop_step = t->steps_done;
    }
    p.stamps = (long long *)(t->ws + t->oT);
}
}  // namespace

extern "C" {

size_t cem_trainer_workspace_bytes(const cem_train_config_t *cfg)
{
    if (validate_train(cfg)) return 0;
    cem_trainer t; t.cfg = *cfg; train_layout(&t); return t.total;
}
size_t cem_trainer_blob_floats(const cem_train_config_t *cfg) { return validate_train(cfg) ? 0 : train_nat(cfg) * cfg->ensemble_size; }

int cem_trainer_create(const cem_train_config_t *cfg, void *workspace, size_t workspace_bytes, void *hip_stream, cem_trainer_t **out)
{
    int st = validate_train(cfg); if (st) return st;
    if (!workspace || !out) return CEM_ERR_INVALID_ARG;
    cem_trainer *t = new (std::nothrow) cem_trainer();
    if (!t) return CEM_ERR_INVALID_ARG;
    t->cfg = *cfg; train_layout(t);
    if (workspace_bytes < t->total || ((uintptr_t)workspace & 255)) { delete t; return CEM_ERR_WORKSPACE; }
    t->ws = (char *)workspace; t->stream = (hipStream_t)hip_stream; t->own_stream = false;
    if (!t->stream) {
        if (hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking) != hipSuccess) { g_last_hip = (int)hipGetLastError(); delete t; return CEM_ERR_HIP; }
        t->own_stream = true;
    }
    if (hipMemsetAsync(t->ws, 0, t->total, t->stream) != hipSuccess || hipStreamSynchronize(t->stream) != hipSuccess) {
        g_last_hip = (int)hipGetLastError(); delete t; return CEM_ERR_HIP;
    }
    {   // the tile kernel keeps every layer's activations in LDS: (n_layers + 5) x 8 KB, beyond 48 KB only with the runtime's leave
        const size_t lds = (size_t)(cfg->n_layers + 5) * CEM_TT_NB * CEM_TT_BLK;
        t->tile_kernel = cfg->n_layers <= CEM_TT_MAXL && cfg->units <= CEM_U && cfg->activation == CEM_ACT_RELU && cfg->dropout_rate == 0.f &&
                         std::getenv("CEM_TRAIN_GEMM_KERNEL") == nullptr;   // the tile kernel is 8 blocks wide and relu only
        hipError_t e = hipSuccess;
        if (t->tile_kernel) switch (cfg->n_layers) {
#define CEM_CASE(LL) case LL: e = tile_kernel_lds<LL>(lds); break;
            CEM_CASE(1) CEM_CASE(2) CEM_CASE(3) CEM_CASE(4) CEM_CASE(5) CEM_CASE(6)
#undef CEM_CASE
        }
        if (e != hipSuccess) { (void)hipGetLastError(); t->tile_kernel = false; }
    }
    *out = t;
    return CEM_OK;
}

int cem_trainer_destroy(cem_trainer_t *t)
{
    if (!t) return CEM_ERR_INVALID_ARG;
    if (t->own_stream) hipStreamDestroy(t->stream);
    if (t->eval_part) hipFree(t->eval_part);
    delete t;
    return CEM_OK;
}

int cem_trainer_set_state(cem_trainer_t *t, const float *weights, const float *m, const float *v)
{
    if (!t || !weights) return CEM_ERR_INVALID_ARG;
    const size_t bytes = t->nat * t->cfg.ensemble_size * 4;
    HIPCHK(hipMemcpyAsync(t->ws + t->oW, weights, bytes, hipMemcpyHostToDevice, t->stream));
    if (m) HIPCHK(hipMemcpyAsync(t->ws + t->oM, m, bytes, hipMemcpyHostToDevice, t->stream)); else HIPCHK(hipMemsetAsync(t->ws + t->oM, 0, bytes, t->stream));
    if (v) HIPCHK(hipMemcpyAsync(t->ws + t->oV, v, bytes, hipMemcpyHostToDevice, t->stream)); else HIPCHK(hipMemsetAsync(t->ws + t->oV, 0, bytes, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    // (steps_done is NOT reset: the Dropout masks are a function of the step index since create, so a trainer whose weights are
    // re-staged from outside — every fit of an agent loop — goes on to fresh masks instead of replaying the first ones)
    return CEM_OK;
}

int cem_trainer_get_state(cem_trainer_t *t, float *weights, float *m, float *v)
{
    if (!t) return CEM_ERR_INVALID_ARG;
    const size_t bytes = t->nat * t->cfg.ensemble_size * 4;
    if (weights) HIPCHK(hipMemcpyAsync(weights, t->ws + t->oW, bytes, hipMemcpyDeviceToHost, t->stream));
    if (m) HIPCHK(hipMemcpyAsync(m, t->ws + t->oM, bytes, hipMemcpyDeviceToHost, t->stream));
    if (v) HIPCHK(hipMemcpyAsync(v, t->ws + t->oV, bytes, hipMemcpyDeviceToHost, t->stream));
    HIPCHK(hipStreamSynchronize(t->stream));
    return CEM_OK;
}

int cem_trainer_weights_dev(cem_trainer_t *t, const float **blob_dev_out, size_t *n_floats_out)
{
    if (!t || !blob_dev_out || !n_floats_out) return CEM_ERR_INVALID_ARG;
    *blob_dev_out = (const float *)(t->ws + t->oW);
    *n_floats_out = t->nat * t->cfg.ensemble_size;
    return CEM_OK;
}

int cem_trainer_step(cem_trainer_t *t, const float *x_dev, const float *y_dev, const int32_t *perm_dev, int32_t nperm, int32_t offset,
                     int32_t bt, float lr_t, float *loss_dev)
{
    if (!t || !x_dev || !y_dev || !loss_dev || bt < 1 || bt > t->cfg.batch_size || offset < 0) return CEM_ERR_INVALID_ARG;
    if (perm_dev && offset + bt > nperm) return CEM_ERR_INVALID_ARG;
    TrainParams p; fill_train_params(t, p);
    p.x = x_dev; p.y = y_dev; p.perm = perm_dev; p.nperm = nperm; p.offset = offset; p.Bt = bt; p.chunk = bt; p.lr_t = lr_t; p.loss_out = loss_dev; p.train = 1;
    p.nparts = train_parts(bt);
    launch_train_step(t, p);
    t->steps_done += 1;
    const size_t n4 = (size_t)p.E * p.nat / 4;
    const unsigned adam_grid = (unsigned)std::min<size_t>(std::max<size_t>((n4 + 255) / 256, 1), 2048);
    hipLaunchKernelGGL(cem_adam_kernel, dim3(adam_grid), dim3(256), 0, t->stream, p);
    HIPCHK(hipGetLastError());
    return CEM_OK;
}

int cem_trainer_steps(cem_trainer_t *t, const float *x_dev, const float *y_dev, const int32_t *perm_dev, int32_t nperm, int32_t n_steps,
                      const int32_t *offsets, const int32_t *bts, const float *lr_ts, float *loss_dev)
{
    if (!t || !offsets || !bts || !lr_ts || n_steps < 0) return CEM_ERR_INVALID_ARG;
    for (int s = 0; s < n_steps; ++s) {
        const int st = cem_trainer_step(t, x_dev, y_dev, perm_dev, nperm, offsets[s], bts[s], lr_ts[s], loss_dev + (size_t)s * t->cfg.ensemble_size);
        if (st) return st;
    }
    return CEM_OK;
}

int cem_trainer_eval(cem_trainer_t *t, const float *x_dev, const float *y_dev, int32_t n, float *loss_out)
{
    if (!t || !x_dev || !y_dev || !loss_out || n < 1) return CEM_ERR_INVALID_ARG;
    const int E = t->cfg.ensemble_size;
    std::vector<float> sums((size_t)E * 2);
    std::fill(sums.begin(), sums.end(), 0.f);
    TrainParams p; fill_train_params(t, p);
    p.x = x_dev; p.y = y_dev; p.perm = nullptr; p.loss_out = (float *)(t->ws + t->oL); p.train = 0;
    const int B = eval_chunk_rows(t->cfg), nchunks = (n + B - 1) / B;
    const int P = train_parts(B);                   // <= 4: a chunk of at most 64 rows, one 16-row pass per part
    const size_t per_chunk = (size_t)E * P * 2;
    std::vector<float> part(per_chunk * (t->tile_kernel ? nchunks : 1));
    // the sums are added on the host in the same order either way: chunk by chunk, member by member, part by part
    auto add_chunk = [&](const float *pc, int rows) {
        const int nparts = (rows + CEM_TROWS - 1) / CEM_TROWS;
        for (int m = 0; m < E; ++m)
            for (int q = 0; q < nparts; ++q) { sums[2 * m] += pc[((size_t)m * P + q) * 2]; sums[2 * m + 1] += pc[((size_t)m * P + q) * 2 + 1]; }
    };
    if (t->tile_kernel) {
        // ONE launch for the whole set: grid.y walks the 64-row chunks, each writing its own loss partials
        if (t->eval_part_floats < part.size()) {
            if (t->eval_part) { HIPCHK(hipStreamSynchronize(t->stream)); HIPCHK(hipFree(t->eval_part)); t->eval_part = nullptr; t->eval_part_floats = 0; }
            HIPCHK(hipMalloc((void **)&t->eval_part, part.size() * 4)); t->eval_part_floats = part.size();
        }
        p.chunk = B; p.nparts = P;
        const int kMaxChunks = 32768;                   // grid.y is limited to 65535: very large sets go in several launches
        for (int c0 = 0; c0 < nchunks; c0 += kMaxChunks) {
            const int nc = std::min(kMaxChunks, nchunks - c0);
            p.offset = c0 * B; p.Bt = std::min(n - c0 * B, nc * B); p.loss_part = t->eval_part + (size_t)c0 * per_chunk;
            launch_train_step(t, p);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(part.data(), t->eval_part, part.size() * 4, hipMemcpyDeviceToHost, t->stream));
        HIPCHK(hipStreamSynchronize(t->stream));
        for (int ch = 0; ch < nchunks; ++ch) add_chunk(part.data() + (size_t)ch * per_chunk, std::min(B, n - ch * B));
    } else {
        for (int off = 0; off < n; off += B) {
            p.offset = off; p.Bt = std::min(B, n - off); p.chunk = p.Bt; p.nparts = P;
            launch_train_step(t, p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(part.data(), t->ws + t->oP, part.size() * 4, hipMemcpyDeviceToHost, t->stream));
            HIPCHK(hipStreamSynchronize(t->stream));
            add_chunk(part.data(), p.Bt);
        }
    }
    const double cnt = (double)n * t->cfg.outputs_dim;
    double total = 0;
    for (int m = 0; m < E; ++m) total += (0.5 * sums[2 * m] / cnt + 0.5 * sums[2 * m + 1] / cnt) / E;
    *loss_out = (float)total;
    return CEM_OK;
}

int cem_trainer_forward(cem_trainer_t *t, const float *x_dev, int32_t n_rows, int32_t map, const float *eps_dev, uint64_t seed, uint64_t call,
                        float *mu_out_dev, float *var_out_dev, float *sd_out_dev, float *sample_out_dev)
{
    if (!t || !x_dev || n_rows < 1 || (map != CEM_FORWARD_SPLIT && map != CEM_FORWARD_ALL)) return CEM_ERR_INVALID_ARG;
    if (!mu_out_dev && !var_out_dev && !sd_out_dev && !sample_out_dev) return CEM_ERR_INVALID_ARG;
    const cem_train_config_t &c = t->cfg;
    const int E = c.ensemble_size;
    if (map == CEM_FORWARD_SPLIT && n_rows % E != 0) return CEM_ERR_SPLIT;
    ForwardParams p;
    std::memset(&p, 0, sizeof(p));
    p.W = (const float *)(t->ws + t->oW); p.x = x_dev; p.eps = sample_out_dev ? eps_dev : nullptr;
    p.mu = mu_out_dev; p.var = var_out_dev; p.sd = sd_out_dev; p.sample = sample_out_dev;
    p.rpm = map == CEM_FORWARD_ALL ? n_rows : n_rows / E; p.all = map == CEM_FORWARD_ALL;
    p.D = c.inputs_dim; p.O = c.outputs_dim; p.U = c.units; p.L = c.n_layers; p.E = E; p.nat = (uint32_t)t->nat; p.act = c.activation;
    // the key of cem_philox_words: (seed_lo, seed_hi ^ call_hi), counter word 3 = call_lo
    p.key.k0 = (uint32_t)seed; p.key.k1 = (uint32_t)(seed >> 32) ^ (uint32_t)(call >> 32); p.key.c3 = (uint32_t)call;
    const long long ntiles = ((long long)p.rpm + CEM_TROWS - 1) / CEM_TROWS;
    // the Philox counter holds the output row in 32 bits; a launch grid holds fewer than 2^32 threads
    if ((long long)E * p.rpm > 0xffffffffll || E > 65535 || ntiles * E * (64 * CEM_TT_WAVES) > 0xffffffffll) return CEM_ERR_UNSUPPORTED;
    // the tile form is 8 blocks wide and relu only, with one instantiation per layer count (dropout plays no part in inference)
    const bool tile = c.n_layers <= CEM_TT_MAXL && c.units <= CEM_U && c.activation == CEM_ACT_RELU && std::getenv("CEM_TRAIN_GEMM_KERNEL") == nullptr;
    if (tile) {
        const size_t lds = (size_t)2 * CEM_TT_NB * CEM_TT_BLK;
        const dim3 grid((unsigned)ntiles, (unsigned)E);
        switch (c.n_layers) {
#define CEM_CASE(LL) case LL: hipLaunchKernelGGL((cem_trainer_forward_tile_kernel<LL>), grid, dim3(64 * CEM_TT_WAVES), lds, t->stream, p); break;
        CEM_CASE(1) CEM_CASE(2) CEM_CASE(3) CEM_CASE(4) CEM_CASE(5) CEM_CASE(6)
#undef CEM_CASE
        }
    } else {
        // one scratch slot of a training step per workgroup (five of its L + 8 matrices are used); a workgroup walks its member's tiles
        p.scratch = (float *)(t->ws + t->oS); p.scratch_per_member = (uint32_t)t->scratch_pm; p.ts = c.units > CEM_TS ? CEM_TWIDE : CEM_TS;
        p.nslots = (int)std::min<long long>(train_parts_alloc(c), ntiles);
        hipLaunchKernelGGL(cem_trainer_forward_gemm_kernel, dim3((unsigned)(E * p.nslots)), dim3(CEM_TNT), 0, t->stream, p);
    }
    HIPCHK(hipGetLastError());
    return CEM_OK;
}

}  // extern "C"
