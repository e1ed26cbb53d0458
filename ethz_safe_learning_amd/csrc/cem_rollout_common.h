// cem_rollout_common.h — what the rollout kernels share around their dense stages: cem_rollout_tile (cem_device.h),
// the chunked tile (cem_rollout_chunked.h: the split and bf16 kernels), cem_rollout_wide_kernel (cem_rollout_wide.h) and the
// lean kernels (cem_rollout_lean.hip, cem_rollout_lean_straight.hip) differ in how a dense stage is computed and in where a stage's input travels; the action loads,
// the model noise, the rare scorer kinds and the reward / cost / done bookkeeping are written ONCE, here, at file scope, and every
// name they touch is an argument (nothing is captured from the expanding function).
// They are macros, not functions: the rollout kernels are tuned to their register counts, and as forceinline functions these pieces
// moved vgpr_count in 32 of the 42 rollout instantiations (tests/test_warm_capi_cpu.py pins them); as macros the device code is
// unchanged to the byte (profiles/rollout_common_isa.txt).
// Not a header of its own: cem_device.h includes it at the head of its rollout section, below the types and primitives it uses.
#pragma once

// This lane's actions of step TN_ in the quad of input block W_ + 4 I_, row chunk C_.  MODE_ 0: the padded quad layout (one 16-byte
// buffer load per unit and step, the step in the scalar offset; ACT_RS_ / ACTV_ = buffer and per-(block, chunk) byte offsets);
// MODE_ 1 (caller-supplied action tensors): the natural [n][H][A] layout, element by element (ACTROW_ = the chunks' rows).
#define CEM_LOAD_ACT(DST, MODE_, P_, ACT_RS_, ACTV_, ACTROW_, W_, Q_, O_, A_, I_, C_, TN_) do { \
        if ((MODE_) == 0) DST = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(ACT_RS_, ACTV_[I_][C_], (TN_) * (P_).act_nq * 16, 0)); \
        else { _Pragma("unroll") for (int r = 0; r < 4; ++r) { \
            int af = 16 * ((W_) + 4 * (I_)) + 4 * (Q_) + r - (O_); af = af < 0 ? 0 : (af >= (A_) ? (A_) - 1 : af); \
            DST[r] = ACTROW_[C_][(TN_) * (A_) + af]; } } } while (0)

// The model noise of step T_ for the feature quad Q_ of block FO_ of one row (SLOT_): the caller's eps_model tensor (MODE_ 1, parity
// mode; TREAD_ is the step it is read at, B_ the problem of a batched plan) or Philox keyed on the GLOBAL (row, step, iteration, quad).
// sampling_propagation False: exactly 0 either way (RSCALE_ = 0).
#define CEM_MODEL_NOISE4(DST, MODE_, P_, TD_, B_, O_, T_, TREAD_, SLOT_, FO_, Q_, KEY_, RSCALE_) do { \
        if ((MODE_) == 1 && (P_).eps_model) { \
            const int f0 = 16 * (FO_) + 4 * (Q_); \
            _Pragma("unroll") for (int r = 0; r < 4; ++r) { \
                const int fc = (f0 + r < (O_)) ? f0 + r : (O_) - 1; \
                DST[r] = (P_).eps_model[(B_) * (P_).eps_model_pstride + ((size_t)(TREAD_) * (P_).Btot + (TD_).noise_row_base + (SLOT_)) * (O_) + fc]; \
            } \
            DST = DST * ((P_).sampling ? 1.0f : 0.0f); \
        } else { \
            DST = cem_normal4((uint32_t)((TD_).noise_row_base + (SLOT_)), (uint32_t)(T_), (uint32_t)(P_).it, \
                              (uint32_t)(4 * (FO_) + (Q_)), CEM_STREAM_MODEL, KEY_, RSCALE_); \
        } } while (0)

// reward / cost / done bookkeeping of step T_ from the scorer terms in PART_ (rows of the tile on the lanes of the bookkeeping wave
// WBK_); T_ = -1 only initialises D_PREV_ / C_PREV_ from s_0.  NK_ = 1 + constrained cost kinds, CSZ_ their sizes, IND_CAP_ / CLIPV_
// the indicator cap / reward clip (+inf: none), COST_RS_ the problem's cost bytes.  The order of the done update against the return
// is the reference's, and differs between the variants.
#define CEM_PART_MIN4(PART_, LANE_, K_) fminf(fminf((PART_)[((K_) * 4 + 0) * 64 + (LANE_)], (PART_)[((K_) * 4 + 1) * 64 + (LANE_)]), \
                                              fminf((PART_)[((K_) * 4 + 2) * 64 + (LANE_)], (PART_)[((K_) * 4 + 3) * 64 + (LANE_)]))
#define CEM_BOOKKEEP(P_, TD_, PART_, W_, WBK_, LANE_, NK_, CSZ_, IND_CAP_, CLIPV_, COST_RS_, D_PREV_, C_PREV_, CUM_, DONE_, T_) do { if ((W_) == (WBK_)) { \
        const float dn = CEM_PART_MIN4(PART_, LANE_, 0); \
        float cn = 0.f; \
        _Pragma("unroll") for (int k = 1; k < CEM_NKIND; ++k) \
            if (k < (NK_)) { const float dk = CEM_PART_MIN4(PART_, LANE_, k); cn = cn + ((dk <= (CSZ_)[k - 1]) ? 1.0f : 0.0f); } \
        cn = fminf(cn, IND_CAP_);                                  /* constrain_indicator: cost > 0 -> 1 (cn is a count) */ \
        if ((T_) >= 0) { \
            const bool ga = D_PREV_ <= (P_).sc.goal_thresh;                               /* safety_gym.py:116 */ \
            float r = (D_PREV_ - dn) * (P_).sc.reward_distance + (ga ? 1.0f : 0.0f) * (P_).sc.reward_goal; \
            r = fminf(fmaxf(r, -(CLIPV_)), CLIPV_);                    /* reward_clip (safety_gym.py:141); +inf: none */ \
            if ((P_).variant == 1) {                                                      /* safe_cem_mpc.py:86-93 */ \
                DONE_ = DONE_ || ga; \
                const float nd = DONE_ ? 0.0f : 1.0f; \
                const float cst = C_PREV_ * nd; \
                if ((P_).costs && (LANE_) < (TD_).cnt) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)cst, COST_RS_, (TD_).row_base + (LANE_), __builtin_amdgcn_readfirstlane((T_) * (P_).Bloc), 0); \
                CUM_ = CUM_ + r * nd; \
            } else {                                                                      /* mpc_policy.py:34-37 */ \
                const float nd = DONE_ ? 0.0f : 1.0f; \
                CUM_ = CUM_ + r * nd; \
                DONE_ = DONE_ || ga; \
            } } \
        D_PREV_ = dn; C_PREV_ = cn; } } while (0)

// min over the 4 lane rows that hold different features of the same batch row, for TWO scorer kinds at once: one row swap
// puts kind KA's partial minima into the even lane rows and kind KA+1's into the odd ones, one half swap finishes both (two
// VALU swaps + two v_min for a pair of kinds, no LDS).  Lane rows 0 / 2 then hold kind KA, rows 1 / 3 kind KA + 1 (PAIRED)
// and every row stores its kind's value for its batch row (rows q and q + 2 store the same word).
#define CEM_PAIR_MIN_STORE(PART_, W_, Q_, J_, KA, VA, VB, PAIRED, C_) do { \
        const auto r16_ = __builtin_amdgcn_permlane16_swap(__float_as_uint(VA), __float_as_uint(VB), false, false); \
        const uint32_t m16_ = __float_as_uint(fminf(__uint_as_float(r16_[0]), __uint_as_float(r16_[1]))); \
        const auto r32_ = __builtin_amdgcn_permlane32_swap(m16_, m16_, false, false); \
        (PART_)[(((KA) + ((PAIRED) ? ((Q_) & 1) : 0)) * 4 + (W_)) * 64 + 16 * (C_) + (J_)] = fminf(__uint_as_float(r32_[0]), __uint_as_float(r32_[1])); \
    } while (0)

// Publishes a step's scorer terms: PM_ = the running minima of (goal, first cost kind) from cem_scorer_terms, S_ the state registers.
// Scorer kinds beyond those two and the observe_goal_dist form of the goal kind are computed here: rare, kept out of the hot block.
// SEL0_ROW_(SEL0_SRC_, byte offset of the lane's quad in a table row) -> that quad of row CEM_ET_SEL0: out of LDS in the tuned
// kernel (CEM_SEL0_LDS, cem_device.h), from memory in the other two (CEM_SEL0_MEM).
#define CEM_SEL0_MEM(ET_RS_, TV_) cem_ld_tab(ET_RS_, (TV_), CEM_ET_SEL0 * 512)
#define CEM_RARE_KINDS_AND_STORE(RC_, NFW_, P_, PART_, W_, Q_, J_, NK_, S_, PM_, TAB_V_, SEL0_ROW_, SEL0_SRC_) do { \
        if ((P_).sc.goal_mode) {                              /* squeeze(relu(goal_dist)), safety_gym.py:172-174 */ \
            _Pragma("unroll") for (int c = 0; c < (RC_); ++c) PM_[0][c] = __builtin_inff(); \
            _Pragma("unroll") for (int i = 0; i < (NFW_); ++i) { \
                const f4 selg = SEL0_ROW_(SEL0_SRC_, (TAB_V_) + 256 * i); \
                _Pragma("unroll") for (int c = 0; c < (RC_); ++c) \
                    _Pragma("unroll") for (int r = 0; r < 4; ++r) PM_[0][c] = fminf(PM_[0][c], fmaxf(fmaxf(S_[i][c][r], 0.f), selg[r])); } } \
        _Pragma("unroll") for (int c = 0; c < (RC_); ++c) CEM_PAIR_MIN_STORE(PART_, W_, Q_, J_, 0, PM_[0][c], PM_[1][c], true, c); \
        if ((NK_) > 2) {                                      /* vases + hazards + pillars + gremlins all constrained */ \
            float pk[3][RC_]; \
            _Pragma("unroll") for (int k = 0; k < 3; ++k) _Pragma("unroll") for (int c = 0; c < (RC_); ++c) pk[k][c] = __builtin_inff(); \
            _Pragma("unroll") for (int i = 0; i < (NFW_); ++i) { \
                const int f0 = 16 * ((W_) + 4 * i) + 4 * (Q_); \
                _Pragma("unroll") for (int k = 2; k < CEM_NKIND; ++k) if (k < (NK_)) { \
                    const f4 selk = *reinterpret_cast<const f4 *>((P_).kind_sel + k * CEM_U + f0); \
                    _Pragma("unroll") for (int c = 0; c < (RC_); ++c) \
                        _Pragma("unroll") for (int r = 0; r < 4; ++r) { \
                            const float lid = fminf(fmaxf((P_).sc.D - (P_).sc.D * (1.0f - S_[i][c][r]), 0.f), (P_).sc.D); \
                            pk[k - 2][c] = fminf(pk[k - 2][c], fmaxf(lid, selk[r])); } } } \
            _Pragma("unroll") for (int c = 0; c < (RC_); ++c) { \
                CEM_PAIR_MIN_STORE(PART_, W_, Q_, J_, 2, pk[0][c], pk[1][c], true, c); \
                if ((NK_) > 4) CEM_PAIR_MIN_STORE(PART_, W_, Q_, J_, 4, pk[2][c], pk[2][c], false, c); } } } while (0)
