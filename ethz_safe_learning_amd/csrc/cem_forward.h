// cem_forward.h — ensemble inference on the trainer's weights: MlpEnsemble.forward / __call__ (simba/models/mlp_ensemble.py:122-132,
// 189-193) and the member x row map of validation_step (:150-154), returning the heads instead of a loss.
//
// Tile form (cem_trainer_forward_tile_kernel): the forward half of cem_train_tile.h.  A workgroup of 8 waves takes 16 rows of ONE member through
// the L hidden layers and the two heads as chains of v_mfma_f32_16x16x4_f32; wave w owns 16-feature block w of every activation matrix,
// the activations stay in LDS in the accumulator layout, and the weights come straight from the trainer's natural [in][out] blob with
// that file's stage-ahead buffer loads (tt_op / tt_load / tt_mfma are used as they are).  Without a backward pass only the layer being
// read and the layer being written are alive: two activation matrices of 8 blocks (18 KB of LDS instead of the (L + 5) x 9 KB of a
// training pass), no gradient, loss or partial-sum storage, no dropout (training=False).
//
// Row maps (cem_mpc.h enum cem_forward_map), rpm = rows per member:
//   SPLIT  tf.split(x, E) (mlp_ensemble.py:123-126): rpm = n_rows / E, member m reads and writes rows [m rpm, (m + 1) rpm)
//   ALL    every member on every row (:150-154): rpm = n_rows, member m reads rows [0, n_rows) and writes rows [m n_rows, (m + 1) n_rows)
// so in both maps OUTPUT row = m rpm + local row, and the input row is that (SPLIT) or the local row (ALL).
//
// Epilogue on the heads' accumulators: mu as it is; var = softplus(v) + 1e-4 with the training loss's own train_softplus, so forward
// returns what training_step sees; sd = sqrt(var); sample = mu + sd * eps, one rounding per operation (-ffp-contract=off).  eps comes from
// a tensor in the output's shape or from cem_normal4 (cem_device.h) at counter (idx = output row, t = iteration = 0, sub = feature quad,
// stream CEM_STREAM_MODEL).  Every output pointer may be null; no noise is drawn unless a sample is asked for.
//
// Generic form (cem_trainer_forward_gemm_kernel): what the tile form does not cover (units 129..256, activations other than relu, more than
// CEM_TT_MAXL layers) runs the forward GEMMs of cem_train_step_kernel (wg_gemm, same epilogue operands) in the trainer's scratch, one
// slot per workgroup as in a training step; a workgroup takes every nslots-th 16-row tile of its member, so any row count is one launch.
#pragma once
#include "cem_device.h"
#include "cem_train_tile.h"

struct ForwardParams {
    const float *W;              // [E][nat] weights (natural blob layout of cem_mpc.h)
    const float *x;              // [n_rows][D] inputs, already scaled
    const float *eps;            // noise in the sample's shape, or null: Philox
    float *mu, *var, *sd, *sample;       // [E * rpm][O] each, or null
    float *scratch;              // generic form: [E * nslots][scratch_per_member]
    int32_t rpm, all;            // rows per member; all != 0: the ALL map
    int32_t D, O, U, L, E;
    uint32_t nat, scratch_per_member;
    int32_t nslots, ts, act;     // generic form: scratch slots per member, row stride of the activation matrices, enum cem_activation
    PhiloxKey key;
};

// heads -> outputs for element (output row, feature o): m = the mu head's accumulator, v = the variance head's
__device__ __forceinline__ void fwd_emit(const ForwardParams &p, const size_t at, const float m, const float v, const float e)
{
    const float var = train_softplus(v) + 1e-4f;
    if (p.mu) p.mu[at] = m;
    if (p.var) p.var[at] = var;
    if (p.sd || p.sample) {
        const float sd = sqrtf(var);
        if (p.sd) p.sd[at] = sd;
        if (p.sample) p.sample[at] = m + sd * e;
    }
}

template <int L>
__global__ __launch_bounds__(64 * CEM_TT_WAVES) void cem_trainer_forward_tile_kernel(const ForwardParams p)
{
    extern __shared__ __attribute__((aligned(16))) char fsm[];     // [2][8 blocks]: layer l reads matrix l & 1 and writes the other
    const int tid = threadIdx.x, D = p.D, O = p.O, U = p.U;
    const int m = blockIdx.y, row0 = (int)blockIdx.x * CEM_TROWS;
    const int cnt = p.rpm - row0 < CEM_TROWS ? p.rpm - row0 : CEM_TROWS;
    TtCtx c; c.lane = tid & 63; c.q = c.lane >> 4; c.j = c.lane & 15; c.w = __builtin_amdgcn_readfirstlane(tid >> 6); c.cnt = cnt; c.acc = 0;
    const gcptr W = (gcptr)(p.W + (size_t)m * p.nat);
    auto offW = [&](int l) { return l == 0 ? (size_t)0 : (size_t)D * U + U + (size_t)(l - 1) * ((size_t)U * U + U); };
    auto offb = [&](int l) { return offW(l) + (size_t)(l == 0 ? D : U) * U; };
    const size_t oWmu = (size_t)D * U + U + (size_t)(L - 1) * ((size_t)U * U + U), obmu = oWmu + (size_t)U * O;
    const size_t oWv = obmu + O, obv = oWv + (size_t)U * O;
    const int nbU = (U + 15) >> 4, nbO = (O + 15) >> 4;
    const bool own = c.w < nbU, ownO = c.w < nbO;                  // this wave has hidden-unit block w / head block w (wave-uniform)
    const int mb = 16 * c.w;

    // stage s's weights sit in wb[s & 1] and are requested during stage s - 1 (stages 0..L-1 the hidden layers, L the heads)
    float wb[2][CEM_TT_NB][2][4];
    auto fwd_op = [&](const int l) { return tt_op(W + offW(l), (l == 0 ? D : U) * U, U, 1, mb, U, c); };
    { TtOp op[1] = {fwd_op(0)}; if (own) tt_load<1>(wb[0], op); }
    f4 bias[L], bias_mu4, bias_v4;
#pragma unroll
    for (int l = 0; l < L; ++l)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int o = mb + 4 * c.q + r; bias[l][r] = W[offb(l) + (o < U ? o : 0)]; }
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int o = mb + 4 * c.q + r; bias_mu4[r] = W[obmu + (o < O ? o : 0)]; bias_v4[r] = W[obv + (o < O ? o : 0)]; }

    // this lane's row: lanes past the tile's last row repeat it (their results are never stored)
    const int lrow = row0 + (c.j < cnt ? c.j : cnt - 1);
    const size_t in_row = (p.all ? (size_t)0 : (size_t)m * p.rpm) + lrow, out_row = (size_t)m * p.rpm + lrow;
    const bool live = c.j < cnt;
    f4 e = (f4){0.f, 0.f, 0.f, 0.f};                               // the sample's noise, requested now, needed after the heads
    if (p.sample && p.eps && ownO) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int o = mb + 4 * c.q + r; e[r] = p.eps[out_row * O + (o < O ? o : O - 1)]; }
    }
    {   // h_0: wave w brings input block w (features past the input width: zeros)
        f4 x;
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int f = mb + 4 * c.q + r; x[r] = f < D ? p.x[in_row * D + f] : 0.f; }
        *reinterpret_cast<f4 *>(fsm + c.w * CEM_TT_BLK + CEM_TT_LANE(c)) = x;
    }
    __syncthreads();

#pragma unroll
    for (int l = 0; l < L; ++l) {
        if (l + 1 < L) { TtOp op[1] = {fwd_op(l + 1)}; if (own) tt_load<1>(wb[(l + 1) & 1], op); }
        else {
            TtOp op[2] = {tt_op(W + oWmu, U * O, O, 1, mb, O, c), tt_op(W + oWv, U * O, O, 1, mb, O, c)};
            if (ownO) tt_load<2>(wb[(l + 1) & 1], op);
        }
        f4 acc[1];
#pragma unroll
        for (int r = 0; r < 4; ++r) { const int o = mb + 4 * c.q + r; acc[0][r] = o < U ? bias[l][r] : 0.f; }
        if (own) tt_mfma<1>(acc, wb[l & 1], fsm + (size_t)(l & 1) * CEM_TT_NB * CEM_TT_BLK, c);
        f4 h = acc[0];
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = (mb + 4 * c.q + r < U) ? fmaxf(h[r], 0.f) : 0.f;     // units past U stay exactly zero
        *reinterpret_cast<f4 *>(fsm + (size_t)((l + 1) & 1) * CEM_TT_NB * CEM_TT_BLK + c.w * CEM_TT_BLK + CEM_TT_LANE(c)) = h;
        __syncthreads();
    }
    if (!ownO) return;                                             // wave-uniform, after the last barrier

    // Philox noise does not depend on the heads: drawn before their MFMA chain is waited for
    if (p.sample && !p.eps) e = cem_normal4((uint32_t)out_row, 0u, 0u, (uint32_t)(4 * c.w + c.q), CEM_STREAM_MODEL, p.key);
    f4 acc[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) { const int o = mb + 4 * c.q + r; acc[0][r] = o < O ? bias_mu4[r] : 0.f; acc[1][r] = o < O ? bias_v4[r] : 0.f; }
    tt_mfma<2>(acc, wb[L & 1], fsm + (size_t)(L & 1) * CEM_TT_NB * CEM_TT_BLK, c);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = mb + 4 * c.q + r;
        if (live && o < O) fwd_emit(p, out_row * O + o, acc[0][r], acc[1][r], e[r]);
    }
}

// ---- generic form: the forward GEMMs of cem_train_step_kernel, then the same epilogue -----------------------------------------------
__global__ __launch_bounds__(CEM_TNT) void cem_trainer_forward_gemm_kernel(const ForwardParams p)
{
    const int m = blockIdx.x / p.nslots, slot = blockIdx.x % p.nslots;
    const int D = p.D, O = p.O, U = p.U, L = p.L, S = p.ts;
    const float *W = p.W + (size_t)m * p.nat;
    float *sc = p.scratch + (size_t)blockIdx.x * p.scratch_per_member;
    // scratch carve (a training step's slot holds L + 8 such matrices): h_0, two hidden matrices used in turn, the two heads
    float *xs = sc, *ha = xs + CEM_TROWS * S, *hb = ha + CEM_TROWS * S, *mu = hb + CEM_TROWS * S, *vp = mu + CEM_TROWS * S;
    auto offW = [&](int l) { return l == 0 ? (size_t)0 : (size_t)D * U + U + (size_t)(l - 1) * ((size_t)U * U + U); };
    auto offb = [&](int l) { return offW(l) + (size_t)(l == 0 ? D : U) * U; };
    const size_t oWmu = (size_t)D * U + U + (size_t)(L - 1) * ((size_t)U * U + U), obmu = oWmu + (size_t)U * O;
    const size_t oWv = obmu + O, obv = oWv + (size_t)U * O;
    const int ntiles = (p.rpm + CEM_TROWS - 1) / CEM_TROWS;
    for (int tile = slot; tile < ntiles; tile += p.nslots) {       // (workgroup-uniform)
        const int row0 = tile * CEM_TROWS;
        const int Bt = p.rpm - row0 < CEM_TROWS ? p.rpm - row0 : CEM_TROWS;
        const size_t in0 = (p.all ? (size_t)0 : (size_t)m * p.rpm) + row0, out0 = (size_t)m * p.rpm + row0;
        if (tile != slot) __syncthreads();                         // the tile before is done with the scratch
        wg_map<float>(Bt * S,
            [&](int e) { const int r = e / S, c = e % S; return c < D ? p.x[(in0 + r) * D + c] : 0.f; },
            [&](int e, float v) { xs[e] = v; });
        __syncthreads();
        const float *hin = xs;
        for (int l = 0; l < L; ++l) {
            float *hout = (l & 1) ? hb : ha;
            GemmEpi fe{(gptr)hout, S, (gcptr)(W + offb(l)), nullptr, 0, 1 + p.act, nullptr, nullptr, nullptr, nullptr, nullptr};
            wg_gemm(Bt, U, l == 0 ? D : U, (gcptr)hin, S, 1, (gcptr)(W + offW(l)), U, 1, fe, CEM_NOSPLIT);
            hin = hout;
        }
        // both heads as ONE GEMM: columns [0, O) = mu head, [O, 2O) = variance head
        wg_gemm(Bt, 2 * O, U, (gcptr)hin, S, 1, (gcptr)(W + oWmu), O, 1,
                GemmEpi{(gptr)mu, S, (gcptr)(W + obmu), nullptr, 0, 0, (gptr)vp, (gcptr)(W + obv), nullptr, nullptr, nullptr}, GemmSplit{nullptr, (gcptr)(W + oWv), 0x7fffffff, O});
        wg_map<float2>(Bt * O,
            [&](int e) { const int r = e / O, c = e % O; return make_float2(mu[r * S + c], vp[r * S + c]); },
            [&](int e, float2 in) {
                const int r = e / O, c = e % O;
                const size_t at = (out0 + r) * O + c;
                float z = 0.f;
                if (p.sample) {
                    if (p.eps) z = p.eps[at];
                    else {
                        const f4 n4 = cem_normal4((uint32_t)(out0 + r), 0u, 0u, (uint32_t)(c >> 2), CEM_STREAM_MODEL, p.key);
                        z = (c & 3) == 0 ? n4[0] : ((c & 3) == 1 ? n4[1] : ((c & 3) == 2 ? n4[2] : n4[3]));
                    }
                }
                fwd_emit(p, at, in.x, in.y, z);
            });
    }
}
