/*
 * cem_mpc.h — C ABI of the MI355X-native CEM-MPC planner (libcem_mpc_gfx950.so).
 *
 * Drop-in boundary for ONE path of yardenas/ethz-safe-learning ("simba"):
 *   CemMpc.generate_action / do_generate_action      simba/policies/cem_mpc.py:31-68
 *   SafeCemMpc.compute_objective                     simba/policies/safe_cem_mpc.py:76-120
 *   MpcPolicy.compute_objective / sampling_params    simba/policies/mpc_policy.py:26-57
 *   TransitionModel.unfold_sequences / scale         simba/models/transition_model.py:64-87
 *   MlpEnsemble.forward / __call__                   simba/models/mlp_ensemble.py:122-132,189-193
 *   SafetyGymStateScorer.reward / cost ('goal' task) simba/environment_utils/safety_gym.py:110-192
 *
 * The reference is pure Python on TensorFlow; it has no FFI of its own.  These
 * entry points are what a ctypes binding inside simba/policies/cem_mpc.py would
 * call (INTEGRATION.md shows that binding).  Plain pointers and sizes only; no
 * torch types.  Device memory (the workspace, optional noise tensors) is owned
 * by the caller (torch-ROCm tensors or hipMalloc), the HIP stream is the
 * caller's.  Every function returns an int status (CEM_OK == 0); nothing
 * throws across the boundary.  A handle is not thread-safe; one plan in flight
 * per handle (the reference has one synchronous caller, simba/agents/agent.py:120);
 * a batch handle plans many observations in that one call (cem_planner_plan_batch).
 * A shape change (scripts/tune_cem_policy.py:109-115) = a new handle.
 *
 * Environment variables the library reads (none changes a result; all are diagnostics or deployment overrides):
 *   CEM_RCCL_LIBRARY=<file>        the RCCL to dlopen instead of librccl.so.1 (a site's build; the tests' shared-memory stand-in).  No
 *                                  fallback if it does not load; logged on stderr whenever it is honoured.
 *   CEM_FORCE_SAMPLER=tile|kernel  where cem_mpc.py:44-48 runs: as the rollout tiles' prologue or as a launch of its own (default: by the
 *                                  tile plan, see cem_planner_launches_per_iteration).
 *   CEM_ASSUME_CUS=<n>             price tile plans for n compute units (the GPU-less host helpers default to 256).  It moves the tile
 *                                  PLAN only (tile size, pinned / floating split — bit-identical results either way); residency decisions
 *                                  (the fused select's grid, where the sampler runs) always use the device's real multiProcessorCount.
 *   CEM_NO_POLL                    cem_planner_plan waits for a captured plan with hipStreamSynchronize instead of polling the result block in
 *                                  pinned memory (polling spins one host core for the duration of the plan and returns ~10 us sooner).
 *   CEM_FORCE_GENERIC_ROLLOUT      every configuration on the width-generic rollout kernel (a CEM_PRECISION_BF16 configuration is refused
 *                                  while it is set, CEM_ERR_UNSUPPORTED: that kernel multiplies in fp32);  CEM_TRAIN_GEMM_KERNEL: the GEMM-by-GEMM trainer.
 */
#ifndef CEM_MPC_H
#define CEM_MPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CEM_ABI_VERSION 4
#define CEM_MAX_ACT 32
#define CEM_MAX_COST_KINDS 4
#define CEM_MAX_BATCH 256         /* problems of one batch handle (cem_batch_planner_create) */

enum cem_status {
    CEM_OK = 0,
    CEM_ERR_INVALID_ARG = 1,     /* NULL pointer / bad dims */
    CEM_ERR_UNSUPPORTED = 2,     /* e.g. units > 256, task 'push', obs+act > 128 */
    CEM_ERR_SPLIT = 3,           /* (particles*n_samples) % ensemble_size != 0: tf.split would raise (mlp_ensemble.py:123) */
    CEM_ERR_WORKSPACE = 4,       /* workspace too small / misaligned */
    CEM_ERR_HIP = 5,             /* a HIP runtime call failed; cem_last_hip_error() has the code */
    CEM_ERR_NO_WEIGHTS = 6,      /* plan() before set_weights() */
    CEM_ERR_STATE = 7,           /* stepwise calls out of order, or a call that would clobber the state of a plan in flight */
    CEM_ERR_COMM = 8,            /* librccl could not be opened, or an RCCL call failed (cem_last_hip_error() holds the ncclResult_t) */
    CEM_ERR_DEVICE = 9           /* a kernel reported that it could not finish its work (a floating rollout segment never received its
                                    work-queue entry within the spin bound; or a fused select's barrier expired AND its recovery did not
                                    run): the plan's result is not valid */
};

/* CEM_VARIANT_COST: SafeCemMpc.optimize_for_safety (safe_cem_mpc.py:40-74) — the same CEM loop on the objective -compute_mean_costs
 * (:98-108): score[n] = -(sum over particles p and steps t < H of cost(s_t) of row p N + n) / P, the cost NOT masked by done.  Scores are
 * <= 0, the planner maximises them (i.e. minimises the mean cost) and the best score it returns is such a negative mean.  Costs are small
 * integers, so the sums are exact and the division by P is the only rounding.  One rank only (world_size > 1: CEM_ERR_UNSUPPORTED);
 * posterior_mean_threashold is ignored.  The rollout of such a handle is the safe variant's launch with a goal threshold that is never
 * reached: cem_layout_t::costs holds the un-masked per-step cost bytes, and what it leaves in cem_layout_t::returns holds nothing (it is
 * neither a reward sum of the reference nor read by anything).  Workspace and tile plan are those of CEM_VARIANT_SAFE at the same shape. */
enum cem_variant { CEM_VARIANT_CEM = 0 /* CemMpc */, CEM_VARIANT_SAFE = 1 /* SafeCemMpc */, CEM_VARIANT_COST = 2 /* SafeCemMpc.optimize_for_safety */ };

/* mlp_params['activation'] of config/models.yaml:12, which the reference `eval`s (mlp_ensemble.py:14): the hidden layers'
 * nonlinearity.  relu (the shipped value) runs on the tuned kernels; the others on the generic rollout kernel and the
 * GEMM-by-GEMM trainer.  tf.nn.elu: alpha 1; tf.nn.leaky_relu: alpha 0.2; tf.nn.selu: scale 1.0507..., alpha 1.6732...; tf.nn.swish (= silu):
 * z sigmoid(z); tf.nn.gelu: the exact form z Phi(z) (approximate=False) — TensorFlow's defaults.  Up to selu the derivative is a function
 * of the layer's OUTPUT, which is what the trainer keeps; swish / gelu are not monotone, so for them the trainer keeps the pre-activations too. */
enum cem_activation { CEM_ACT_RELU = 0, CEM_ACT_TANH = 1, CEM_ACT_SIGMOID = 2, CEM_ACT_ELU = 3, CEM_ACT_LEAKY_RELU = 4, CEM_ACT_SOFTPLUS = 5, CEM_ACT_SELU = 6,
                      CEM_ACT_SWISH = 7, CEM_ACT_GELU = 8 };

/* SafetyGymStateScorer fields used by the 'goal' task (safety_gym.py:104-176).
 * The constants come from safety_gym's Engine config (absent from the
 * reference tree), hence explicit. */
typedef struct cem_scorer {
    int32_t goal_mode;            /* 0: observe_goal_lidar (closest_distance over goal slice); 1: observe_goal_dist (relu of one feature) */
    int32_t goal_lo, goal_hi;     /* sensor_offset_table['goal_lidar'|'goal_dist'] */
    float lidar_max_dist;
    float goal_size;
    float goal_reached_dist;      /* the threshold of `goal_achieved = dist <= 0.8 * goal_size` (safety_gym.py:116) as the reference
                                   * rounds it: the Python-float product converted to an fp32 tensor, fl32(0.8 * goal_size) evaluated in
                                   * double — NOT fl32(goal_size) * 0.8, which is 1 ulp higher at the default goal_size 0.3 */
    float reward_distance;
    float reward_goal;
    float reward_clip;            /* <= 0: no clip (safety_gym.py:141) */
    int32_t constrain_indicator;
    int32_t n_cost_kinds;         /* constrained kinds, reference order vases,hazards,pillars,gremlins (safety_gym.py:148-163) */
    int32_t cost_lo[CEM_MAX_COST_KINDS];
    int32_t cost_hi[CEM_MAX_COST_KINDS];
    float cost_size[CEM_MAX_COST_KINDS];
} cem_scorer_t;

/* How the rollout's dense layers multiply.  All three accumulate in fp32, starting from the fp32 bias; everything outside the dense
 * layers (state, normaliser, heads' outputs, softplus, noise, scorer, bookkeeping) is the same fp32 code in all three.
 * CEM_PRECISION_FP32: v_mfma_f32_16x16x4_f32 (the default; what every number in BASELINE / DESIGN is quoted on unless labelled).
 * CEM_PRECISION_SPLIT_BF16X3: weights and activations as exact three-way bf16 splits, the six leading bf16 x bf16 products per
 * fp32 product on v_mfma_f32_16x16x32_bf16 (csrc/cem_rollout_split.h).  Same oracle, same tolerances, not bit-identical to the
 * fp32 form; units <= 128 and relu only.  These two keep every term of a product down to 2^-24 of it.
 * CEM_PRECISION_BF16: a REDUCED-precision mode (csrc/cem_rollout_bf16.h).  Weights are rounded to bf16 (8 significand bits, round to
 * nearest even) when they are packed, the inputs of every dense stage — the scaled layer-0 input, observation and action features
 * alike, and every post-ReLU hidden activation — where they are published; one v_mfma_f32_16x16x32_bf16 per product block, products
 * exact in its fp32 accumulator.  An operand carries a relative error of up to 2^-8: the results are NOT those of the fp32 form at its
 * tolerances (measured: profiles/bf16_error.json, README); they are those of that rounding model (planner.bf16_reference_forward) at
 * the fp32 kernels' tolerances.  Finite inputs below the largest bf16; units <= 128 and relu only.  Never chosen by the library. */
enum cem_precision { CEM_PRECISION_FP32 = 0, CEM_PRECISION_SPLIT_BF16X3 = 1, CEM_PRECISION_BF16 = 2 };

/* Constructor kwargs of CemMpc / SafeCemMpc (cem_mpc.py:7-17, safe_cem_mpc.py:8-19)
 * + the model dims of TransitionModel/MlpEnsemble (transition_model.py:8-21,
 * config/models.yaml) + candidate sharding. */
typedef struct cem_config {
    int32_t abi_version;          /* CEM_ABI_VERSION */
    int32_t obs_dim, act_dim;
    int32_t units, n_layers;      /* mlp_params: units <= 128 run on the fast kernels (narrower layers zero-padded to the 128-wide form:
                                   * exactly the narrow network's result); 129..256 — and any activation other than relu — on the generic
                                   * kernels (same semantics; cem_rollout_wide.h) */
    int32_t activation;           /* enum cem_activation */
    int32_t ensemble_size;        /* E */
    int32_t particles;            /* P */
    int32_t n_samples;            /* N (global, over all ranks) */
    int32_t horizon;              /* H */
    int32_t n_elite;              /* k */
    int32_t iterations;           /* I */
    float smoothing;
    float one_minus_smoothing;    /* the factor `(1.0 - self.smoothing)` of cem_mpc.py:64-65 as the reference rounds it: a Python-float
                                   * difference converted ONCE to an fp32 tensor, fl32(1.0 - smoothing) evaluated in double — NOT
                                   * 1.0f - fl32(smoothing), which is one ulp off for 41 of the 99 two-decimal smoothing values
                                   * (0.09, 0.16, 0.29, 0.33 ...).  Must lie within 2e-7 of 1 - smoothing (else CEM_ERR_INVALID_ARG) */
    float stddev_threshold;
    float noise_stddev;
    int32_t variant;              /* enum cem_variant */
    float posterior_mean_threashold;   /* sic: the YAML key, config/policies.yaml:20 */
    int32_t sampling_propagation; /* config/agents.yaml:14 */
    int32_t scale_features;       /* config/agents.yaml:13 */
    /* MpcPolicy.sampling_params (mpc_policy.py:45-57), resolved by the caller */
    float act_lb[CEM_MAX_ACT], act_ub[CEM_MAX_ACT], act_mu0[CEM_MAX_ACT], act_sigma0[CEM_MAX_ACT];
    cem_scorer_t scorer;
    /* candidate sharding: this rank owns candidates [rank*N/world, (rank+1)*N/world) x all particles */
    int32_t world_size, rank;
    int32_t chunks_per_tile;      /* 0 = auto; 1..4 = 16-row chunks per workgroup tile */
    int32_t use_graph;            /* 1: capture the whole plan in a hipGraph (single-rank, Philox noise only) */
    int32_t select_mode;          /* 0 = auto; 1 = the one-workgroup select kernel (elite list + 2 H A floats must fit 140 KB of LDS, n_elite <= 24576:
                                   * else CEM_ERR_UNSUPPORTED — auto routes such shapes to 3 / 2 instead); 2 = the multi-workgroup chain of eight launches; 3 = that
                                   * chain as ONE launch with grid barriers: needs its ceil(N / 4096) workgroups resident at once (checked against the
                                   * runtime's occupancy x CU count; else 2 is taken) and is FASTEST on an otherwise idle GPU — CUs held by another
                                   * stream / handle / process or a CU-masked queue can starve a barrier, which then times out (bounded polls, never
                                   * a hang); the launch then commits nothing, a one-workgroup recovery kernel queued right behind it redoes that
                                   * iteration's select from the same scores with mode 2's bits, the plan completes normally (CEM_OK), one line goes
                                   * to stderr and the handle uses mode 2 from then on (cem_planner_select_mode reports it) — what auto picks
                                   * from 24 000 candidates on (the replicated select of a many-GPU plan; below, mode 1 is faster).  Same elite set, best action and
                                   * early stop in every mode; 2 and 3 are bit-identical; mu / sigma of 1 vs 2 / 3 agree to fp32 rounding
                                   * (the moments are summed in a different, still fixed, order).  In every mode equal VALUES tie by candidate
                                   * index, the lower index first (tf.nn.top_k): -0.0 and +0.0 are one value (the best score of a plan whose best
                                   * candidate scored -0.0 may be reported as +0.0; the two compare equal); a NaN score ranks below -inf and is
                                   * never elite while n_elite other candidates exist (fewer than n_elite non-NaN scores: unspecified) */
    int32_t rollout_segments;     /* 0 = auto; 1 = one workgroup per tile for the whole horizon; n > 1 = the rollout launch is a
                                   * work queue of (tile, horizon/n) items drawn by resident workgroups — evens out CU load when the
                                   * tile count is not a multiple of the CU count; results are bit-identical either way */
    int32_t precision;            /* enum cem_precision: how the rollout forms its fp32 products (ABI 4) */
} cem_config_t;

/* Byte offsets into the caller's workspace of the arrays a host binding needs
 * (torch views for the collective, debug outputs). */
typedef struct cem_layout {
    size_t scores_local;   /* float [N/world]   — this rank's candidate scores (input to the collective) */
    size_t scores_global;  /* float [N]         — all candidates' scores (output of the collective; == scores_local slot for world 1) */
    size_t actions;        /* float [N][H][A]   — the current iteration's clipped action sequences */
    size_t mu_sigma;       /* float [2][H][A]   — sampling mean, stddev */
    size_t elite_idx;      /* int32 [k]         — elite set of the last select, ascending index */
    size_t returns;        /* float [P*N/world] — per-row done-masked return of the last rollout (CEM_VARIANT_COST: nothing, see enum cem_variant) */
    size_t costs;          /* uint8 [H][P*N/world] — per-step masked cost (safe variant); the un-masked cost (CEM_VARIANT_COST) */
    size_t result;         /* uint32 [38]: the last completed plan's result as the final kernel left it, word for word the pinned-host block
                            * cem_planner_plan reads: [0, A) action (float), [32] best score (float), [33] iterations run, [34] early-stop
                            * flag, [35] fault bits, [36] the handle's plan counter, [37] checksum.  Valid after the handle's stream has
                            * drained (see cem_planner_plan) */
    size_t stamps;         /* int64 [tiles][4][8] — cycle stamps of the last rollout; written only by -DCEM_STAMPS diagnostic builds */
    size_t total;
    /* the weights as the rollout kernels read them (test / debug views; written by set_weights and set_weights_dev alike) */
    size_t wpack, wpack_bytes;   /* the members' packed weight images; wide shapes: the natural blobs, then the images */
    size_t bias_h;         /* float [E][L][128]  — hidden-layer biases, zero padded (tuned and split kernels) */
    size_t bias_mu, bias_var;    /* float [E][128] each */
    size_t etab, etab_bytes;     /* float [E][rows][128] — the per-member feature table: normaliser, head and hidden-layer biases, masks */
} cem_layout_t;

typedef struct cem_planner cem_planner_t;

int cem_abi_version(void);
const char *cem_status_string(int status);
int cem_last_hip_error(void);

/* natural (Keras) weight blob: per member m, in order
 *   W_0[obs+act][U], b_0[U], W_1[U][U], b_1[U], ... W_{L-1}, b_{L-1},
 *   W_mu[U][obs], b_mu[obs], W_var[U][obs], b_var[obs]        (all row-major [in][out], mlp_ensemble.py:13,28-29) */
size_t cem_weight_blob_floats(const cem_config_t *cfg);
size_t cem_packed_weight_floats(const cem_config_t *cfg);
size_t cem_workspace_bytes(const cem_config_t *cfg);

/* host-only helpers (no GPU needed; exercised by the CPU test-suite) */
int cem_pack_weights_host(const cem_config_t *cfg, const float *blob, float *packed);
int cem_plan_tiles_host(const cem_config_t *cfg, int32_t *chunks_per_tile_out, int32_t *n_tiles_out,
                        int32_t *tiles_out /* [n_tiles][6]: row_base,cnt,member,act_base,noise_row_base,s0_base */, int32_t max_tiles);
/* horizon segments the rollout launch of this configuration uses (1 = unsegmented), as cem_planner_create would choose */
int cem_plan_segments_host(const cem_config_t *cfg, int32_t *segments_out, int32_t *steps_per_segment_out);

/* diagnostic: workgroups of the rollout kernels for (chunks_per_tile, obs+act <= 64 ? 1 : 2 input blocks per wave) one CU keeps
 * resident — what the tile-size choice assumes (`table_out[2]`) and what the HIP runtime reports (`runtime_out[2]`, 0 without a
 * device); element 0: one workgroup per tile, element 1: the pinned + floating-segment launch form. */
int cem_rollout_residency(int32_t chunks_per_tile, int32_t input_blocks_per_wave, int32_t *table_out, int32_t *runtime_out);

/* lifecycle.  `workspace` is device memory of >= cem_workspace_bytes(cfg), 256-B aligned; `hip_stream` a hipStream_t (NULL = default). */
int cem_planner_create(const cem_config_t *cfg, void *workspace, size_t workspace_bytes, void *hip_stream, cem_planner_t **out);
int cem_planner_destroy(cem_planner_t *h);
int cem_planner_layout(const cem_planner_t *h, cem_layout_t *out);

/* weight / normaliser sync after MlpEnsemble.fit and TransitionModel._fit_statistics
 * (mlp_ensemble.py:143-144, transition_model.py:42-50).  Host pointers. */
int cem_planner_set_weights(cem_planner_t *h, const float *blob, size_t n_floats);
int cem_planner_set_normaliser(cem_planner_t *h, const float *inputs_min, const float *inputs_max /* [obs+act] */);
/* The same weight sync from DEVICE memory (after a fit the weights already live there: cem_trainer_weights_dev): the images are packed
 * by kernels (csrc/cem_pack.h), bit for bit what cem_planner_set_weights uploads.
 * blob_dev: E members x cem_weight_blob_floats / E floats in DEVICE memory, the layout cem_planner_set_weights takes on the host.
 * Enqueued on the planner's stream and NOT synchronised: plans queued afterwards on that stream see the new weights, a captured graph
 * stays valid (the images keep their addresses), the warm-start carry is kept (as set_weights keeps it).  The source must stay
 * unchanged until the stream has passed the call; ordering against another stream is the caller's business.
 * CEM_ERR_INVALID_ARG for a NULL handle or pointer or a wrong n_floats, before any device call. */
int cem_planner_set_weights_dev(cem_planner_t *h, const float *blob_dev, size_t n_floats);

/* CemMpc.generate_action (cem_mpc.py:31-33): state[obs] (host) -> action[act] (host).
 * Noise: Philox4x32-7 keyed (seed, call) when the eps pointers are NULL, otherwise explicit
 * DEVICE tensors eps_act[I][N][H][A], eps_model[I][H][P*N][obs] and HOST eps_out[A]
 * (parity mode: "identical seeds" == identical noise tensors).
 * Ordering: a captured plan (use_graph) returns as soon as its result block has landed in pinned host memory (sequence number +
 * checksum), which can be BEFORE the handle's stream has drained.  What it hands back on the host — action, score, iterations — is
 * complete; the DEVICE arrays of cem_layout_t — mu_sigma, elite_idx, scores, actions, result — are ordered only by the stream: a
 * caller that reads them synchronises the handle's stream first (the Python binding's accessors do).  cem_planner_destroy drains
 * the stream itself. */
int cem_planner_plan(cem_planner_t *h, const float *state, uint64_t seed, uint64_t call,
                     const float *eps_act_dev, const float *eps_model_dev, const float *eps_out_host,
                     float *action_out, float *best_score_out, int32_t *iters_out);

/* the same plan split at its one exchange step, for candidate-sharded ranks:
 *   begin; for it: rollout(it) -> [collective on scores_local -> scores_global] -> select(it); end */
int cem_plan_begin(cem_planner_t *h, const float *state, uint64_t seed, uint64_t call,
                   const float *eps_act_dev, const float *eps_model_dev);
int cem_plan_rollout(cem_planner_t *h, int32_t it);   /* sample actions, roll out + score this rank's candidates -> scores_local */
int cem_plan_select(cem_planner_t *h, int32_t it);    /* top-k / moments refit / best-so-far / early-stop on scores_global */
int cem_plan_end(cem_planner_t *h, const float *eps_out_host, float *action_out, float *best_score_out, int32_t *iters_out);

/* The exchange step inside the library: an RCCL communicator owned by the handle, so that a candidate-sharded
 * plan runs without the host between its kernels — cem_planner_plan() then works for world_size > 1 (rollout ->
 * ncclAllGather of the N/world local scores on the handle's stream -> select, per iteration) and, with use_graph, replays
 * it as ONE hipGraph per rank including the collectives.  librccl is opened at run time (dlopen), not linked.
 * Rank 0 calls cem_comm_unique_id() and hands the 128 bytes to the other ranks by any means (torch.distributed broadcast,
 * MPI, a file); every rank then calls cem_planner_comm_init() — collectively, like ncclCommInitRank.
 * cem_plan_exchange() is the same all-gather for the stepwise API (between cem_plan_rollout and cem_plan_select). */
#define CEM_COMM_ID_BYTES 128
int cem_comm_unique_id(void *id_out /* CEM_COMM_ID_BYTES */);
int cem_planner_comm_init(cem_planner_t *h, const void *id /* CEM_COMM_ID_BYTES */, int32_t n_ranks, int32_t rank);
int cem_planner_comm_destroy(cem_planner_t *h);
/* ranks of the handle's communicator as RCCL itself reports them (ncclCommCount); 0 without a communicator */
int cem_planner_comm_ranks(const cem_planner_t *h, int32_t *n_ranks_out);
int cem_plan_exchange(cem_planner_t *h);
/* The select form the handle's next iteration takes (1 / 2 / 3, see cem_config_t::select_mode): what automatic resolves to on this device,
 * and 2 once a fused select has had to be recovered on this handle. */
int cem_planner_select_mode(const cem_planner_t *h, int32_t *mode_out);
/* Which form of the one-workgroup select iteration `it` launches: 0 = the bucket kernel of csrc/cem_device.h (and every select that is not one workgroup);
 * 1 = the ranked kernel of csrc/cem_select_ranked.hip, which keeps a thread's keys in registers and takes five barrier phases in
 * front of the moments — where the select resolves to mode 1 with its keys staged in LDS, n_samples <= 4096 and the objective is
 * CemMpc's.  Same results bit for bit; cem_planner_select_mode reports 1 for both.  CEM_FORCE_SELECT=bucket at create keeps an eligible
 * handle on form 0.  CEM_ERR_INVALID_ARG: `it` outside [0, iterations). */
int cem_planner_select_form(const cem_planner_t *h, int32_t it, int32_t *form_out);
/* The same rule without a handle or a device, for a requested select_mode, a population, an elite count, horizon x act_dim and a variant,
 * on a device that grants the one-workgroup select its 140 KB of dynamic LDS: what cem_planner_select_form reports on such a handle
 * unless CEM_FORCE_SELECT=bucket was set.  CEM_ERR_INVALID_ARG: a select_mode outside 0 .. 3, sizes below 1, n_elite > n_samples. */
int cem_select_form_for(int32_t select_mode, int64_t n_samples, int64_t n_elite, int64_t horizon_x_act_dim, int32_t variant, int32_t *form_out);
/* Test hook.  kind 1: in the NEXT plan's first iteration, the last workgroup of the fused select treats its first grid barrier as
 * expired (as if its peers were not resident) — the recovery path then runs without having to load the GPU.  No effect on plans
 * whose select is not fused.
 * kind 2: the next hipGraph capture cem_planner_plan attempts on this handle counts as refused by the runtime — the path a communicator
 * takes on a stack without captured collectives: that plan and all later ones launch kernel by kernel (graph_status 2), same results. */
int cem_planner_inject_fault(cem_planner_t *h, int32_t kind);
/* 0: cem_planner_plan launches kernel by kernel; 1: it replays a captured hipGraph; 2: capturing was tried and is not supported
 * with this communicator / runtime (the plan then stays kernel by kernel — same results) */
int cem_planner_graph_status(const cem_planner_t *h, int32_t *status_out);
/* Nodes of the captured plan as the runtime counts them (hipGraphGetNodes); 0 while no graph is held (graph_status 0 / 2, or a setter
 * dropped it and no plan has captured anew). */
int cem_planner_graph_nodes(const cem_planner_t *h, int32_t *nodes_out);
/* Kernel launches one CEM iteration of cem_planner_plan takes on this handle (the collective of a sharded plan not counted):
 * 2 = rollout (its tiles sample their own action sequences, cem_mpc.py:44-48) + select (which forms the particle mean of the CemMpc
 * objective itself, mpc_policy.py:38-39) — single-rank CemMpc plans whose tiles are all resident at once; + 1 where the sampler is a
 * launch of its own (tiles queue for slots), + 1 where the reduce kernel stays (SafeCemMpc's Beta filter, sharded plans, the
 * multi-workgroup selects; CEM_VARIANT_COST: its own reduce, csrc/cem_score.h; CEM_PARTICLES_LOWER_TAIL: its reduce, csrc/cem_score.h, which no select folds), + 1 for select_mode 3's recovery kernel (returns at once unless a barrier expired), + 7 for select_mode 2's
 * chain.  The stepwise calls always launch the reduce kernel. */
int cem_planner_launches_per_iteration(const cem_planner_t *h, int32_t *launches_out);
/* Which rollout kernels cem_planner_plan launches on this handle when the plan is given no explicit noise tensors: 0 = the generic
 * kernels; 1 = the lean one-chunk kernels (csrc/cem_rollout_lean.hip), which draw every action in the lane that needs it instead of
 * reading a stored sample — fp32, one chunk per tile, obs + act <= 64 with obs a multiple of 4, single rank, single state, all tiles
 * resident at once.  Same results bit for bit; CEM_FORCE_ROLLOUT=generic at create keeps an eligible handle on the generic kernels.
 * A plan with eps_act / eps_model tensors always runs the generic kernels. */
int cem_planner_rollout_path(const cem_planner_t *h, int32_t *path_out);
/* Which form of them iteration `it` launches: 0 = the generic kernels; 1 = the lean kernels' branchy form (csrc/cem_rollout_lean.hip,
 * every plan fact tested in the step loop); 2 = their straight-line form (csrc/cem_rollout_lean_straight.hip: the objective a template
 * parameter, the weight ring's positions constants), which serves the lean plans whose scorer has its goal as a lidar kind and at most
 * one constrained cost kind.  Same results bit for bit; CEM_FORCE_ROLLOUT=lean_branchy at create keeps an eligible handle on form 1.
 * cem_planner_rollout_path and cem_iteration_plan_t.rollout_path report 1 for both lean forms.  CEM_ERR_INVALID_ARG: `it` outside
 * [0, iterations). */
int cem_planner_rollout_form(const cem_planner_t *h, int32_t it, int32_t *form_out);

/* TransitionModel.unfold_sequences (transition_model.py:64-77) as an API of its own:
 * s0[B][obs], actions[B][H][A] (device) -> traj[B][H+1][obs] (device); optional mu/stddev[B][H][obs].
 * Row r uses member r / (B/E).  Noise: eps_model_dev[H][B][obs] or Philox (seed, call). */
int cem_unfold_sequences(cem_planner_t *h, const float *s0_dev, const float *actions_dev, int32_t n_rows, int32_t horizon,
                         const float *eps_model_dev, uint64_t seed, uint64_t call,
                         float *traj_out_dev, float *mu_out_dev, float *sd_out_dev);

/* MpcPolicy.compute_objective (mpc_policy.py:26-39) / SafeCemMpc.compute_objective (safe_cem_mpc.py:76-96) as an op of its
 * own, on a GIVEN trajectory tensor: traj[n_rows][horizon+1][obs] (device), row r = p * (n_rows / particles) + candidate
 * (the tf.tile order of cem_mpc.py:49-51) -> scores[n_rows / particles] (device).  Uses the handle's variant, particles,
 * posterior threshold and scorer; `horizon` need not be the handle's.  The planner's own rollouts never call this (their
 * objective is the rollout kernel's epilogue and the trajectory is never materialised); it serves callers that hold a
 * trajectory tensor, e.g. from cem_unfold_sequences.
 * On a CEM_VARIANT_COST handle this is SafeCemMpc.compute_mean_costs (safe_cem_mpc.py:98-108) with the SIGN of the planner's objective:
 * scores[n] = -(mean over particles of the summed un-masked cost) <= 0; the reference's (positive) mean costs are their negation.
 * With CEM_PARTICLES_LOWER_TAIL set (cem_planner_set_particle_objective) the particle returns are aggregated that way here too. */
int cem_compute_objective(cem_planner_t *h, const float *traj_dev, int32_t n_rows, int32_t horizon, float *scores_out_dev);

/* MbrlSafetyGym.get_reward / get_cost (safety_gym.py:62-66) -> SafetyGymStateScorer.reward / cost (:110-166), 'goal' task:
 * obs[n][obs], next_obs[n][obs] (device) -> reward[n] (float), goal_achieved[n] (uint8; may be NULL); obs -> cost[n] (float). */
int cem_scorer_reward(cem_planner_t *h, const float *obs_dev, const float *next_obs_dev, int32_t n, float *reward_out_dev,
                      uint8_t *goal_achieved_out_dev);
int cem_scorer_cost(cem_planner_t *h, const float *obs_dev, int32_t n, float *cost_out_dev);

/* dump the Philox streams a (seed, call) plan consumes, in the explicit-tensor layouts above (device pointers; any may be NULL) */
int cem_fill_noise(cem_planner_t *h, uint64_t seed, uint64_t call, float *eps_act_dev, float *eps_model_dev, float *eps_out_dev);

/* The generator behind those streams, word for word (test hook): the four Philox4x32-7 output words of the n counters
 *   (idx0 + i,  t | iteration << 16,  sub | stream << 16,  call & 0xffffffff),  key (seed & 0xffffffff, (seed >> 32) ^ (call >> 32)),
 * written to words_out_dev[n][4] (uint32).  stream: 0 model noise (idx = global batch row, sub = feature quad), 1 action noise
 * (idx = candidate, sub = action quad), 2 output noise (idx = action quad, t = iteration = sub = 0).  Four normals of a counter:
 *   u_k = fl32(fl32(word_k) * 2^-32 + 2^-33);  z0 = r(u0) cos(2 pi u1), z1 = r(u0) sin(2 pi u1), z2 = r(u2) cos(2 pi u3),
 *   z3 = r(u2) sin(2 pi u3),  r(u) = sqrt(-2 ln u)   (tf.random.normal draws of cem_mpc.py:44-47,68 and mlp_ensemble.py:192-193) */
int cem_philox_words(cem_planner_t *h, uint64_t seed, uint64_t call, uint32_t stream, uint32_t iteration, uint32_t t, uint32_t sub,
                     uint32_t idx0, uint32_t n, uint32_t *words_out_dev);

/* device time (ms) of the rollout kernels of the last plan, measured with HIP events on the handle's stream
 * (enabled by cem_planner_set_timing(h, 1); costs one event pair per launch). */
int cem_planner_set_timing(cem_planner_t *h, int32_t enable);
int cem_planner_last_timing(cem_planner_t *h, float *rollout_ms_total, int32_t *rollout_launches, float *select_ms_total);
/* the same plan's other launches: the particle-mean / Beta-filter kernel (where it is a launch of its own; CEM_VARIANT_COST: its cost reduce) and the sampler launch (where the
 * sampler is not the rollout tiles' prologue); 0 where the plan has no such launch */
int cem_planner_last_timing_detail(cem_planner_t *h, float *reduce_ms_total, float *sampler_ms_total);

/* ---------------------------------------------------------------------------------------------------------------
 * Batched planning: ONE plan call for up to max_batch observations (vectorised environments, evaluation episodes run side by side).
 * A batch handle runs B copies of the single-state plan side by side in one launch per stage — the rollout launch holds every problem's
 * tiles (problem b on its own contiguous block of workgroups), the select one 1024-thread workgroup per problem — and captures them as
 * ONE hipGraph (use_graph) for max_batch problems: any 1 <= n_states <= max_batch is valid on every call, problems n_states .. max_batch - 1
 * are staged as already stopped (no iterations), so varying n_states never re-captures (cem_planner_graph_status stays 1).
 * Problem b returns exactly — bit for bit: action, best score, iterations — what cem_planner_plan(h1, states[b], seed, calls[b], ...)
 * returns on a single-state handle h1 of the same configuration: same Philox counters (keyed (seed, calls[b]); rows and candidates
 * problem-relative), same arithmetic, its own early stop (a problem that has stopped is skipped by every later kernel).  Explicit noise:
 * problem b reads slice b of eps_act[n][I][N][H][A], eps_model[n][I][H][P*N][obs] (device) and eps_out[n][A] (host), each slice laid out
 * as the single-plan tensor.  All problems share the handle's weights, normaliser and scorer.
 *
 * Scope — cem_batch_workspace_bytes returns 0 and cem_batch_planner_create returns the status when:
 *   world_size > 1                                                                CEM_ERR_UNSUPPORTED
 *   precision other than CEM_PRECISION_FP32                                       CEM_ERR_UNSUPPORTED
 *   a shape for the generic rollout kernel (units > 128, activation other than relu, or CEM_FORCE_GENERIC_ROLLOUT set)   CEM_ERR_UNSUPPORTED
 *   select_mode 2 or 3                                                            CEM_ERR_UNSUPPORTED
 *   select_mode 0 that would not resolve to the one-workgroup select (N >= 24 000, or its LDS limit)                    CEM_ERR_UNSUPPORTED
 *   max_batch x (tiles of one problem) beyond the int32 range of a launch grid    CEM_ERR_UNSUPPORTED
 *   max_batch outside 1 .. CEM_MAX_BATCH                                          CEM_ERR_INVALID_ARG
 *   ... and every configuration cem_workspace_bytes rejects, with the same status.
 * Rollout segments: a batch handle runs one workgroup per tile for the whole horizon (rollout_segments is ignored; bit-identical).
 * Its tile size is priced for all max_batch problems' tiles in one launch (chunks_per_tile 0), which need not be the single plan's.
 *
 * Calls that work on a batch handle: set_weights, set_normaliser, layout (per-problem arrays are [max_batch] consecutive slices of the
 * single-plan sizes; result is [max_batch][38]), destroy, graph_status, launches_per_iteration (at most 4, independent of n_states),
 * set_timing / last_timing / last_timing_detail (I rollout launches per batched plan whatever n_states is), select_mode, fill_noise,
 * philox_words.  cem_planner_plan, the stepwise cem_plan_* calls, cem_planner_comm_init and the model ops (unfold_sequences,
 * compute_objective, scorer_reward / scorer_cost) return CEM_ERR_STATE on a batch handle; cem_planner_plan_batch returns
 * CEM_ERR_STATE on a single-state handle.
 * Result: the final kernel writes every problem's block ([b][0 .. 37] as cem_layout_t::result describes one) to pinned host memory, the
 * plan counters last; cem_planner_plan_batch waits for all n_states blocks as cem_planner_plan waits for its one. */
size_t cem_batch_workspace_bytes(const cem_config_t *cfg, int32_t max_batch);            /* 0 if cfg or max_batch is out of scope */
int cem_batch_planner_create(const cem_config_t *cfg, int32_t max_batch, void *workspace, size_t workspace_bytes, void *hip_stream,
                             cem_planner_t **out);
/* states[n_states][obs], calls[n_states] (host); actions_out[n_states][act], best_scores_out[n_states], iters_out[n_states] (host).
 * CEM_ERR_INVALID_ARG for n_states < 1 or > max_batch (the handle stays usable). */
int cem_planner_plan_batch(cem_planner_t *h, int32_t n_states, const float *states, uint64_t seed, const uint64_t *calls,
                           const float *eps_act_dev, const float *eps_model_dev, const float *eps_out_host, float *actions_out,
                           float *best_scores_out, int32_t *iters_out);
int cem_planner_batch_capacity(const cem_planner_t *h, int32_t *max_batch_out);          /* max_batch; 0 for a single-state handle */

/* ---------------------------------------------------------------------------------------------------------------
 * Warm start: where a plan's initial mu / sigma [H][A] come from.  Additive: a handle on which none of
 * these is called plans bit for bit as before (CEM_INIT_COLD, the reference's behaviour: cem_mpc.py:39-40).
 *
 * Every handle keeps a CARRY per slot: mu and sigma [H][A] as the slot's last completed plan left them (after the refit of
 * the last iteration it ran, early stop included) and a valid flag.  A single-state handle has one slot, 0; a batch handle
 * has max_batch slots.  A plan that returns anything but CEM_OK, and cem_planner_reset_carry, make the carry invalid;
 * set_weights / set_normaliser keep it.  The carry becomes valid when the plan call returns CEM_OK (stepwise: at the end call).
 * The model ops (unfold_sequences, compute_objective, the scorer ops) neither read nor change it.
 *
 * The next plan of a slot starts from (mode is sticky per slot until changed):
 *   CEM_INIT_COLD      act_mu0[a], act_sigma0[a] at every step
 *   CEM_INIT_EXPLICIT  the [H][A] arrays uploaded for the slot (none uploaded: CEM_ERR_STATE from the plan call)
 *   CEM_INIT_SHIFT     the carry moved `shift` = s steps towards the present; exactly COLD while the carry is invalid
 *       mu[t]    = carry_mu[t + s]                               t <  H - s
 *                = act_mu0 (tail 0)  or  carry_mu[H - 1] (tail 1) t >= H - s
 *       sigma[t] = act_sigma0                                     sigma_rule 0 (reset), every t
 *                = max(carry_sigma[t + s], sigma_floor[a])        sigma_rule 1 (keep), t <  H - s;  act_sigma0 for t >= H - s
 * Every operation is a copy or a max of two fp32 values: nothing is rounded, a host restatement is exact.
 * All of it happens in the plan's first kernel, from control data staged in pinned memory: changing a mode, the slot map,
 * n_states or the warm-start parameters never re-captures the handle's graph. */
enum cem_init_mode { CEM_INIT_COLD = 0, CEM_INIT_EXPLICIT = 1, CEM_INIT_SHIFT = 2 };
typedef struct cem_warm_start {
    int32_t shift;                   /* 1 .. horizon - 1 */
    int32_t tail;                    /* 0: the box's act_mu0; 1: repeat the carry's last step */
    int32_t sigma_rule;              /* 0: reset to act_sigma0; 1: keep, floored */
    float sigma_floor[CEM_MAX_ACT];  /* per action dimension, >= 0 and finite (read by sigma_rule 1 only) */
} cem_warm_start_t;
/* parameters of CEM_INIT_SHIFT (default: shift 1, tail 0, sigma_rule 0).  CEM_ERR_INVALID_ARG for a shift outside 1 .. H - 1, a tail or
 * sigma_rule other than 0 / 1, a negative or non-finite floor; the handle keeps its previous parameters and stays usable. */
int cem_planner_set_warm_start(cem_planner_t *h, const cem_warm_start_t *ws);
/* mu[H][A], sigma[H][A] (host) of CEM_INIT_EXPLICIT for `slot`: a stream-ordered copy in front of the next plan.  CEM_ERR_INVALID_ARG
 * for a slot out of range, a non-finite value or a negative sigma (nothing is uploaded then).  Does not change the slot's mode. */
int cem_planner_set_initial_distribution(cem_planner_t *h, int32_t slot, const float *mu, const float *sigma);
int cem_planner_set_init_mode(cem_planner_t *h, int32_t slot, int32_t mode);             /* slot -1: every slot */
int cem_planner_reset_carry(cem_planner_t *h, int32_t slot);                             /* slot -1: every slot */
/* the slot's carry to host mu[H][A], sigma[H][A] (either may be NULL) and its valid flag (arrays are zero filled while invalid);
 * waits for the handle's stream; CEM_ERR_STATE between the begin and end calls of a stepwise plan */
int cem_planner_get_carry(cem_planner_t *h, int32_t slot, float *mu, float *sigma, int32_t *valid);
/* Batch handles only (CEM_ERR_STATE otherwise): in the following cem_planner_plan_batch calls problem b reads and writes carry slot slots[b]
 * (default, and slots NULL: b); problems n .. max_batch - 1 take the remaining slots in ascending order.  n is 1 .. max_batch; slots must be
 * distinct and in 0 .. max_batch - 1, else CEM_ERR_INVALID_ARG (the previous map stays).  A slot that takes no part in a call (its problem
 * index is >= that call's n_states) keeps its carry and its mode. */
int cem_planner_set_carry_slots(cem_planner_t *h, int32_t n, const int32_t *slots);

/* ---------------------------------------------------------------------------------------------------------------
 * The particle objective: how the P particle returns of a candidate become its score.  Beyond the reference, off by default.
 *   CEM_PARTICLES_MEAN        the reference's reduce_mean (mpc_policy.py:38-39): what every handle does unless told otherwise, with the
 *                             launches, graph nodes and bits it always had.
 *   CEM_PARTICLES_LOWER_TAIL  the mean of the m SMALLEST of the P returns, CVaR at level m / P (m = 1: the worst particle).  For
 *                             candidate n with r_p = returns[p][n]: order the particles ascending by (r_p, p) — equal returns go in
 *                             particle order —, take the first m, add them in that order as a sequential fp32 sum starting from 0.f,
 *                             divide once by (float)m.  (m = P is therefore the mean summed in ANOTHER order: not MEAN's bits.)
 *                             NaN returns are outside the contract.
 * On a CEM_VARIANT_SAFE handle the Beta filter and the penalty are unchanged and apply to this value: score = value - (unsafe ? 1 : 0) * 100.
 * The rollouts are untouched; one kernel (csrc/cem_score.h) takes the place of the particle-mean kernel, and a plan that folded the
 * mean into its select launches it in addition (cem_planner_launches_per_iteration says so).  Whole plans (graph and eager), the
 * stepwise calls, batch handles, warm start, every rollout family and cem_compute_objective serve it.
 * The setting is sticky per handle; changing it drops the captured graph (the next plan captures again) and waits for the stream.  Back
 * on MEAN the handle gives the bits of one that never left it.
 *   CEM_ERR_INVALID_ARG  null handle, unknown kind, LOWER_TAIL with m outside 1 .. particles (MEAN ignores m)
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  LOWER_TAIL on a CEM_VARIANT_COST handle (a tail of the particle COSTS is not offered there; as a CONSTRAINT on a
 *                        CEM_VARIANT_SAFE handle it is: cem_planner_set_constraint, worst_cost_particles), on a handle whose constraint
 *                        is CEM_CONSTRAINT_BUDGET (a lower tail of the returns within a budget is not offered), on world_size > 1 (the
 *                        kernel is rank-local and would serve a shard; no multi-rank run of it has been made), and for particles > 128
 *                        (the kernel keeps a block's P x 64 returns in LDS and eight particles per wave in registers)
 * The handle keeps its previous setting after any of these. */
enum cem_particle_objective { CEM_PARTICLES_MEAN = 0, CEM_PARTICLES_LOWER_TAIL = 1 };
int cem_planner_set_particle_objective(cem_planner_t *h, int32_t kind, int32_t m);
/* kind and m as set (MEAN: m = 0); either pointer may be NULL */
int cem_planner_get_particle_objective(const cem_planner_t *h, int32_t *kind_out, int32_t *m_out);

/* ---------------------------------------------------------------------------------------------------------------
 * The constraint of a CEM_VARIANT_SAFE handle: what its cost bytes do to a candidate's score.  Beyond the reference, off by default
 * (DESIGN.md 4.9).
 *   CEM_CONSTRAINT_BETA    the reference's per-step Beta filter (safe_cem_mpc.py:90-96,110-120): score = return - (unsafe ? 100 : 0).
 *                          What every handle does unless told otherwise, with the launches, graph nodes and bits it always had.
 *   CEM_CONSTRAINT_BUDGET  constrained CEM (Wen & Topcu 2018): maximise the return subject to `predicted cumulative cost <= budget`.
 *                          For candidate n of problem b, from the done-masked cost bytes costs[H][P][N] and returns[P][N] of the rollout:
 *                            c_p = sum over t of costs[t][p][n]                       an integer
 *                            T   = the sum of the m_c largest c_p                     m_c = worst_cost_particles; 0 or P: every particle,
 *                                                                                     the particle MEAN of the cumulative cost; m_c < P:
 *                                                                                     its upper tail, CVaR at level m_c / P (1: the worst particle)
 *                            C   = (float)T / (float)m_c                              one fp32 division
 *                            feasible iff C <= budget[b]                              in fp32, inclusive
 *                            R   = (((0.f + r_0) + r_1) + ... + r_{P-1}) / (float)P   the particle mean as CEM_CONSTRAINT_BETA forms it
 *                            score = feasible ? R : cem_f32_encode_infeasible(T) = -(float)(2^23 + T) * 2^77
 *                          Infeasible scores are exact, strictly ordered by T and at or below -2^100, so the unchanged select does the
 *                          whole rule: feasible candidates rank by return and, below all of them, infeasible ones by ascending cost
 *                          (ties to the lowest index); the best-so-far (strict >) prefers any feasible candidate to any infeasible one and,
 *                          among infeasible ones, the cheaper.  A mean return at or below -2^100 is outside the contract (reward_clip
 *                          bounds returns far above it).  The Beta filter and posterior_mean_threashold play no part.
 * One kernel (csrc/cem_score.h) takes the place of the particle-mean / Beta kernel: cem_planner_launches_per_iteration is unchanged.
 * Whole plans (graph and eager), the stepwise calls, batch handles, warm start, every rollout family, every select form and
 * cem_compute_objective (which then returns these scores) serve it.  The setting is sticky per handle; a change waits for the stream and
 * drops the captured graph.  Back on BETA the handle launches exactly what it launched before.
 *   CEM_ERR_INVALID_ARG  null handle, unknown kind, BUDGET with worst_cost_particles outside 0 .. particles (BETA ignores it)
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  BUDGET on a CEM_VARIANT_CEM or CEM_VARIANT_COST handle (it needs the SAFE rollout's cost bytes); world_size > 1
 *                        (the kernel is rank-local; no multi-rank run of it has been made); 0 < m_c < particles with particles > 128 (the
 *                        tail form keeps eight particles per wave in registers); horizon * m_c * CEM_MAX_COST_KINDS >= 2^23 (the encoding);
 *                        BUDGET while CEM_PARTICLES_LOWER_TAIL is set (and LOWER_TAIL while BUDGET is set)
 * The handle keeps its previous setting after any of these. */
enum cem_constraint_kind { CEM_CONSTRAINT_BETA = 0, CEM_CONSTRAINT_BUDGET = 1 };
int cem_planner_set_constraint(cem_planner_t *h, int32_t kind, int32_t worst_cost_particles);
/* kind and m_c as they act (BETA: 0; BUDGET: 1 .. particles, the mean form reads back as particles); either pointer may be NULL */
int cem_planner_get_constraint(const cem_planner_t *h, int32_t *kind_out, int32_t *worst_cost_particles_out);
/* budgets[n] (host): n == 1 sets every problem row of the handle, 1 < n <= max_batch rows 0 .. n - 1 of a batch handle.  Default +inf
 * (everything feasible); +-inf are allowed, NaN is CEM_ERR_INVALID_ARG (nothing is written), as are a null pointer and n outside
 * 1 .. max(max_batch, 1); CEM_ERR_STATE between the begin and end calls of a stepwise plan.  The values live in a small device
 * allocation the handle owns (created on first use, not part of the workspace) and are read by the kernel at run time: the write is a
 * stream-ordered copy — plans queued earlier keep the old values, plans queued later see the new ones — and never drops or re-captures
 * the graph.  May be called on any handle and before cem_planner_set_constraint; only CEM_CONSTRAINT_BUDGET reads the values. */
int cem_planner_set_cost_budget(cem_planner_t *h, const float *budgets, int32_t n);
/* C of the first n candidates of `problem` as the last constrained reduce left them (a plan's last iteration, a stepwise rollout, or
 * cem_compute_objective) -> out_host[n].  Drains the handle's stream; may be called inside a stepwise plan.  CEM_ERR_INVALID_ARG for a
 * null handle or pointer, a problem outside the last launch, n < 1 or beyond its candidates; CEM_ERR_STATE when no constrained reduce
 * has run on the handle. */
int cem_planner_constraint_costs(cem_planner_t *h, int32_t problem, float *out_host, int32_t n);

/* The encoding of infeasible scores, both directions (planner.py mirrors them: encode_infeasible, decode_constrained_score).  T < 2^23:
 * (float)(2^23 + T) is an integer below 2^24 and the power of two scales it exactly.
 * On the names: these are inline, not symbols of the library, and every OTHER `cem_<lower-case name>(` of this header is an exported
 * symbol — tests/test_capi_cpu.py checks exactly that by scanning for such names.  The `f32` (the encoding is an fp32 one) keeps the
 * three helpers recognisably apart from the exported calls, for that scan and for a reader. */
#if defined(__HIPCC__)
#define CEM_INLINE static inline __host__ __device__
#else
#define CEM_INLINE static inline
#endif
#define CEM_INFEASIBLE_BELOW (-0x1p100f)          /* feasible iff score > CEM_INFEASIBLE_BELOW */
CEM_INLINE float cem_f32_encode_infeasible(int32_t total) { return -((float)(8388608 + total)) * 0x1p77f; }
CEM_INLINE int cem_f32_score_is_feasible(float score) { return score > CEM_INFEASIBLE_BELOW; }
/* T of an infeasible score (call only where !cem_f32_score_is_feasible(score)) */
CEM_INLINE int32_t cem_f32_decode_infeasible(float score) { return (int32_t)(-score * 0x1p-77f) - 8388608; }

/* ---------------------------------------------------------------------------------------------------------------
 * The refit: what an iteration does with the scores once the k elites are chosen.  Beyond the reference, off by default.
 *   CEM_REFIT_UNIFORM  the reference's update (cem_mpc.py:56-65): every elite counts 1 / k.  What every handle does unless told otherwise,
 *                      with the launches, graph nodes and bits it always had.
 *   CEM_REFIT_SOFTMAX  the score-weighted update of MPPI (n_elite = n_samples) and of "weighted elites" (n_elite < n_samples).  The elite
 *                      set, the best-so-far rule and the iteration count are the select's, unchanged.  Then, for one problem and iteration:
 *                        s_j   = scores[elite[j]],  s_max = max_j s_j           NaN among the elites is outside the contract
 *                        beta  = fl32(1 / temperature)                          rounded once on the host
 *                        w_j   = s_j == s_max ? 1 : expf((s_j - s_max) * beta)   fp32; ties, +-inf and an all -inf elite set take the first
 *                                                                               branch; -inf, or a budget-encoded infeasible score at any
 *                                                                               temperature below 2^93, beside a finite s_max gives 0
 *                        W     = sum w_j (>= 1)
 *                        mean  = sum w_j a_j / W,  var = sum w_j (a_j - mean)^2 / W      two-pass, per column of the [H][A] action rows
 *                        mu    = s mu + fl32(1 - s) mean,  sigma = s sigma + fl32(1 - s) sqrtf(var)     the blend of cem_mpc.py:64-65
 *                        stop iff mean(sigma) <= stddev_threshold                cem_mpc.py:66-67, summed in the select's order
 *                        ESS   = W^2 / sum w_j^2                                 in [1, k]; reported (cem_planner_refit_stats), feeds nothing
 *                      The summation order is fixed (csrc/cem_refit_weighted.h states it) and there are no floating-point atomics: equal
 *                      inputs give equal bits.  As temperature -> inf the weights tend to 1 and the update to UNIFORM's values (not its
 *                      bits: the sums run in another order).
 * One kernel (csrc/cem_refit_weighted.h) runs behind the unchanged one-workgroup select, whose own blend goes to a scratch slice of a small
 * device allocation the handle owns (made on first use; the workspace keeps its layout and size): cem_planner_launches_per_iteration
 * reports one launch more, and the plan's result is written by the final kernel.  Every variant, particle objective, constraint and
 * rollout family serves it (it reads the scores alone), as do batch handles, warm start (the carry is the weighted mu / sigma), graph and
 * eager plans and the stepwise calls.  The setting is sticky per handle; a change (of the temperature alone, too) waits for the stream
 * and drops the captured graph.  Back on UNIFORM the handle launches exactly what it launched before.
 *   CEM_ERR_INVALID_ARG  null handle, unknown kind, SOFTMAX with a temperature that is NaN, infinite, zero or negative (UNIFORM ignores it)
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  SOFTMAX with world_size > 1 or a communicator, with select_mode 2 or 3, or with n_samples large enough that the
 *                        automatic choice is a multi-workgroup select (about 24 000): those forms keep moment kernels of their own
 * The handle keeps its previous setting after any of these. */
enum cem_refit { CEM_REFIT_UNIFORM = 0, CEM_REFIT_SOFTMAX = 1 };
int cem_planner_set_refit(cem_planner_t *h, int32_t kind, float temperature);
/* kind and temperature as set (UNIFORM: 0); either pointer may be NULL */
int cem_planner_get_refit(const cem_planner_t *h, int32_t *kind_out, float *temperature_out);
/* ESS of iterations 0 .. n - 1 of `problem` as the handle's last weighted plan left them -> ess_out_host[n], n <= iterations.  An
 * iteration the plan did not run (early stop) keeps what an earlier plan left there, 0 at first: read `iters` values.  Drains the
 * handle's stream; may be called inside a stepwise plan.  CEM_ERR_INVALID_ARG for a null handle or pointer, a problem outside
 * 0 .. max(max_batch, 1) - 1, n < 1 or n > iterations; CEM_ERR_STATE when no weighted select has run on the handle. */
int cem_planner_refit_stats(cem_planner_t *h, int32_t problem, float *ess_out_host, int32_t n);

/* ---------------------------------------------------------------------------------------------------------------
 * The action noise: what the sampler of cem_mpc.py:44-48 multiplies by sigma.  Beyond the reference, off by default.
 *   CEM_NOISE_WHITE  the reference's tf.random.normal: every step of every sequence independent.  What every handle does unless told
 *                    otherwise, with the launches, graph nodes and bits it always had (the lean rollout where it is eligible).
 *   CEM_NOISE_MIXED  time-correlated ("coloured") noise, eps = M xi: ONE mixing matrix M[H][H] per handle — fp32, row-major, row = output
 *                    step t, column = input step u —, shared by all action dimensions, iterations and problems.  For problem b, iteration
 *                    i, candidate n and action dimension a:
 *                      xi[u]  = cem_normal4(n, u, i, a / 4, CEM_STREAM_ACT, key(b))[a % 4]     the white stream, unchanged: what
 *                                                                                             cem_fill_noise dumps as eps_act
 *                      eps[t] = acc after:  acc = +0.f;  for u = 0 .. H - 1 in order:  acc = fl32(acc + fl32(M[t][u] * xi[u]))
 *                      action = clip(eps[t] * sigma[t][a] + mu[t][a], lb[a], ub[a])           the existing sampler, unchanged
 *                    The multiply and the add are rounded separately, no term is skipped (zeros of M included: a white draw of -0.0
 *                    under M = I comes out as +0.0, the one difference from WHITE, and it vanishes in the action), there are no
 *                    floating-point atomics, and equal inputs give equal bits on every launch.  Model noise, eps_out, the select, the
 *                    refit, the warm start and every objective are as they are.  Any Gaussian correlation along the horizon is such an
 *                    M (planner.py: powerlaw_mixing, ar1_mixing; mix_noise restates the sum above in NumPy, bit for bit).
 * One kernel (csrc/cem_noise_mix.h) runs once per plan behind the plan's first kernel and writes eps[slots][I][N][H][A] into a device
 * allocation the handle owns (made on first use; the workspace keeps its layout and size); the samplers — as the rollout tiles' prologue,
 * as a floating segment's prologue, as a launch of their own — then read it the way they read a caller's eps_act tensor.  The lean kernels
 * draw in place and cannot take a tensor: while MIXED, cem_planner_rollout_path reports the generic path.
 * cem_planner_launches_per_iteration is unchanged; a captured plan gains one node.  Whole plans (graph and eager), the stepwise calls
 * (cem_plan_begin runs the mix), batch handles (one M for all problems; a problem staged as stopped is skipped and its slice of eps keeps
 * its bytes), warm start, every variant, particle objective, constraint, refit and precision serve it.
 * A caller's own eps_act tensor (cem_planner_plan, cem_plan_begin, cem_planner_plan_batch) is taken as given and is NOT mixed.
 * The setting is sticky per handle; the setter waits for the stream and drops the captured graph.  Back on WHITE the handle launches
 * exactly what a fresh handle launches.
 *   CEM_ERR_INVALID_ARG  null handle, unknown kind, MIXED with a NULL matrix, WHITE with a non-NULL matrix, any non-finite entry
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  MIXED with world_size > 1 or a communicator (and cem_planner_comm_init on a MIXED handle); horizon > 128 (the
 *                        kernel keeps M in LDS: 64 KB at 128)
 * A failed allocation returns CEM_ERR_HIP.  The handle keeps its previous setting after any of these. */
enum cem_action_noise { CEM_NOISE_WHITE = 0, CEM_NOISE_MIXED = 1 };
int cem_planner_set_action_noise(cem_planner_t *h, int32_t kind, const float *mix_host /* [H][H] or NULL */);
/* kind as set and, while MIXED, the matrix as set -> mix_out_host[H][H] (WHITE: not written); either pointer may be NULL */
int cem_planner_get_action_noise(const cem_planner_t *h, int32_t *kind_out, float *mix_out_host /* [H][H] or NULL */);
/* The mixed tensor of the handle's last MIXED plan where it lives: a device pointer into the handle's allocation, [slots][I][N][H][A]
 * floats (slots = max(max_batch, 1)), and the float count.  Valid until destroy; contents follow the handle's stream (synchronise before
 * reading); zeros until a MIXED plan has run.  NULL and 0 on a handle that has never been MIXED (it owns no such allocation). */
int cem_planner_action_noise_dev(cem_planner_t *h, const float **eps_dev_out, size_t *n_floats_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Elite carry-over: the best sequences an iteration has evaluated are candidates of the next one, and of the next plan (iCEM's "keep
 * elites" and "shift elites").  Beyond the reference, off by default.
 *   n_keep = m        0: off — what every handle does unless told otherwise, with the launches, graph nodes and bits it always had (the lean
 *                     rollout and the folded sampler where create chose them).  m > 0: see below.
 *   across_plans      0: nothing of an earlier plan is read.  1: the first iteration of a plan takes the previous plan's last kept elites,
 *                     shifted by `shift` steps.
 *   shift = s         steps executed between two plans; read with across_plans only.
 * Every problem of the handle (max(max_batch, 1) of them) owns a store E[m][H][A] of fp32 and an int32 count, in ONE device allocation the
 * handle owns (made by the first enabling call, grown by a call with a larger m, freed at destroy; the workspace keeps its layout and size).
 *   KEEP    one kernel directly behind the select of iteration `it` (behind the weighted refit where that runs).  It acts iff that select
 *           ran (the problem had not stopped before it; the select that stops the plan still keeps).  The k elites are ordered by the score
 *           the select ranked — descending, -0.0 and +0.0 equal, NaN below -inf, ties to the lower candidate index — and
 *           E[j] = actions[e_j] for the first m of them, as exact copies; count = m.
 *   INJECT  one kernel in iteration `it` between the sampler launch and the rollout launch.  Nothing on a stopped problem or count == 0.
 *           With c = count and s_it = (it == 0 ? s : 0): for n < c, t < H - s_it, a < A the action (n, t, a) of the sample is replaced by
 *           E[n][t + s_it][a]; steps t >= H - s_it keep what the sampler drew for candidate n.  Nothing is clipped (stored values are clipped
 *           samples of the same box).  Launched at it >= 1 always, at it == 0 on across_plans handles only, where the device-side count
 *           decides: one captured graph serves the first plan and later ones.
 * A carried sequence is a candidate like any other: rolled out with this iteration's model noise, scored, ranked; it can be elite again,
 * enter the refit and become best-so-far.  mu / sigma, every candidate's Philox counters (rows n < c are drawn, then overwritten), model
 * noise, eps_out, the select, the refit, early stop, best-so-far, warm start and every objective are as they are; an eps_act tensor (a
 * caller's, or the handle's CEM_NOISE_MIXED one) feeds the sampler as before.  Neither kernel does floating-point arithmetic.
 * count is zeroed, in stream order, by cem_planner_reset_carry (its slot), by every call of this setter, and in front of the next plan
 * after any plan call that returned something other than CEM_OK.  cem_planner_set_weights* and cem_planner_set_normaliser keep the stores.
 * While n_keep > 0 the sampler is a launch of its own (cem_sample_kernel) and the rollouts are the generic kernels:
 * cem_planner_rollout_path reports 0 and cem_planner_launches_per_iteration counts the sampler launch where it had been folded, + 1 for the
 * inject, + 1 for the keep.  With cem_planner_set_timing on, the inject's time is part of the sampler time and the keep's part of the select
 * time (cem_planner_last_timing_detail, cem_planner_last_timing).  Tile plan, segments and work queue are unchanged.  Whole plans (graph and eager), the stepwise calls and
 * batch handles (n_keep only) serve it.  The setter waits for the stream and drops the captured graph.
 *   CEM_ERR_INVALID_ARG  null handle or pointer; n_keep < 0, > n_elite or >= n_samples; across_plans not 0 / 1; reserved != 0; with
 *                        across_plans: shift < 1 or >= horizon
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  n_keep > 0 with world_size > 1 or a communicator (and cem_planner_comm_init on an enabled handle), on a handle
 *                        outside the one-workgroup select (select_mode 2 / 3: the rule of cem_planner_set_refit), with n_elite > 4096, or
 *                        with across_plans on a batch handle (its rows move between slots)
 * A failed allocation (the first enabling call, or a call with a larger n_keep than the handle has room for) returns CEM_ERR_HIP.  The
 * handle keeps its previous setting after any of these: off, unless an earlier call enabled it. */
typedef struct { int32_t n_keep, across_plans, shift, reserved; } cem_elite_carry_t;
int cem_planner_set_elite_carry(cem_planner_t *h, const cem_elite_carry_t *carry);
int cem_planner_get_elite_carry(const cem_planner_t *h, cem_elite_carry_t *carry_out);
/* The store and the count of `problem` as the stream leaves them -> out_host[n_keep][H][A], *count_out (either may be NULL, not both).
 * Drains the handle's stream; may be called inside a stepwise plan.  CEM_ERR_STATE on a handle whose carry-over is off. */
int cem_planner_elite_store(cem_planner_t *h, int32_t problem, float *out_host /* [n_keep][H][A] */, int32_t *count_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Per-iteration population sizes (iCEM's population decay) and the mean as a candidate of the last iteration.  Beyond the reference,
 * off by default.
 *
 * cem_planner_set_population_schedule: n[it] is the population of iteration `it`.  NULL / count == 0, or every entry equal to
 * n_samples, is OFF: the handle launches exactly what create chose (the lean rollout and the folded sampler included).  The schedule
 * need not be monotone.  Iteration `it` of a scheduled plan is iteration `it` of a handle created with n_samples = n[it], on the same
 * mu / sigma, best-so-far, seed and call:
 *   plan      tile size, tile list (the row-to-member map (p n[it] + j) / (P n[it] / E), pinned / floating split), horizon segments,
 *             sampler placement, lean eligibility, select caching and reduce folding are those of the n[it]-wide configuration, from the
 *             functions create uses, priced with the handle's chunks_per_tile and rollout_segments.  cem_planner_iteration_plan reports them.
 *   results   candidates are 0 .. n[it] - 1; scores, elite indices, actions and the padded actions occupy the LEADING n[it] entries of
 *             their arrays; nothing beyond them is read or written.
 *   noise     Philox counters are those of the n[it]-wide plan: the candidate index for actions, the global row p n[it] + j for the model.
 *   tensors   eps_act stays [I][N][H][A] with N = n_samples: iteration `it` reads rows j < n[it] of slab `it`.  eps_model stays
 *             [I][H][P N][O]: iteration `it` reads the leading H P n[it] O floats of slab `it` as [H][P n[it]][O] — what the kernels do
 *             when handed the slab's base and P n[it] rows.  The handle's own CEM_NOISE_MIXED tensor is read the same way (its kernel keeps
 *             filling all N rows).  cem_fill_noise is unchanged: it describes the n_samples-wide streams.
 *   the rest  mu / sigma, refit, smoothing, early stop, iters, best-so-far, the result block and the warm-start carry are as they are.
 * No workspace offset or size moves: the tile descriptors of iterations with n[it] != n_samples live in ONE device allocation the handle
 * owns (freed at destroy), and so do the segment flags and the hand-over state when an iteration needs more of them than the base plan.
 * The setter waits for the stream and drops the captured graph; it allocates before it changes anything, so a refused or failed call
 * leaves the handle as it was.  Whole plans (graph and eager), the stepwise calls (cem_plan_rollout(h, it) uses iteration it's plan) and
 * timing handles serve it, with every objective, refit, action noise and carry-over setting.
 *   CEM_ERR_INVALID_ARG  null handle; count not 0 or `iterations`; an entry < n_elite, > n_samples, or with particles * n[it] not a
 *                        multiple of ensemble_size
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  world_size > 1 or a communicator (and cem_planner_comm_init on a scheduled handle); batch handles; handles
 *                        outside the one-workgroup select (the rule of cem_planner_set_refit); an entry <= n_keep while carry-over is on
 *                        (and cem_planner_set_elite_carry with such an n_keep on a scheduled handle)
 * The getter always fills all `iterations` entries (n_samples where the schedule is off) and says through *enabled_out whether one is on. */
int cem_planner_set_population_schedule(cem_planner_t *h, const int32_t *n /* [iterations] or NULL */, int32_t count);
int cem_planner_get_population_schedule(const cem_planner_t *h, int32_t *n_out /* [iterations] */, int32_t count, int32_t *enabled_out);
/* What iteration `it` launches, on every handle, scheduled or not.  `launches` counts by the rule of cem_planner_launches_per_iteration,
 * rollout_path is 1 for the lean kernels and 0 for the generic ones (cem_planner_rollout_path); those two functions keep their meaning
 * and report iteration 0.  n_segments 1: one workgroup per tile; n_pinned: tiles that stay whole. */
typedef struct { int32_t n_samples, chunks_per_tile, n_tiles, n_segments, n_pinned, launches, rollout_path, reserved; } cem_iteration_plan_t;
int cem_planner_iteration_plan(const cem_planner_t *h, int32_t it, cem_iteration_plan_t *out);

/* The mean as a candidate (iCEM): in iteration `iterations - 1` only — a plan that stops early never gets there — one kernel between
 * the sampler launch and the rollout launch (behind the elite inject where that runs) overwrites the LAST candidate of that iteration,
 * row n[I - 1] - 1 of `actions` and its words of the padded layout, with min(max(mu[t][a], lb[a]), ub[a]) from the mu the iteration
 * samples from.  Padding words keep their zeros; no Philox counter moves (the row is drawn, then overwritten).  That iteration samples
 * in a launch of its own and runs the generic rollout, as an iteration with carry-over does (+ 1 launch for the kernel, + 1 where the
 * sampler had been folded); the other iterations keep what they had.  Refusals are those of the schedule's setter, plus
 * CEM_ERR_UNSUPPORTED for n_keep >= n[I - 1] - 1 while carry-over is on (either order of the setters), and CEM_ERR_INVALID_ARG for
 * enable not 0 / 1. */
int cem_planner_set_mean_candidate(cem_planner_t *h, int32_t enable);
int cem_planner_get_mean_candidate(const cem_planner_t *h, int32_t *enable_out);

/* ---------------------------------------------------------------------------------------------------------------
 * Plan read-out: the best-so-far action SEQUENCE and the particle evidence behind it.  Beyond the reference, off by default
 * (DESIGN.md 4.14).  A plan returns the first action of the best sequence, its score and an iteration count; with the read-out on, one
 * more kernel (cem_plan_track_kernel, csrc/cem_plan_readout.h) directly behind every iteration's select — behind the weighted refit and
 * the elite keep where those run — keeps, per problem, in ONE device allocation the handle owns (made by the first enabling call, freed
 * at destroy; the workspace keeps its layout and size):
 *   sequence[H][A]       the best-so-far candidate's whole row of `actions`, an exact copy; sequence[0] is what the plan returns before
 *                        the output noise (noise_stddev * eps_out) is added
 *   score                its score: the plan's best_score
 *   candidate, iteration its index in the population of the iteration that found it, and that iteration; -1 / -1: nothing was found
 *                        (every score was -inf or NaN, or the problem is a batch row that was not live)
 *   particle_returns[P]  ret[q * N_it + candidate], q = 0 .. P - 1, exact copies; N_it is that iteration's population
 *                        (cem_planner_set_population_schedule).  On CEM_VARIANT_CEM with the mean objective
 *                        score == (((0 + r_0) + r_1) + ... + r_{P-1}) / P in fp32, bit for bit.  On CEM_VARIANT_COST these are the returns
 *                        the safe rollout also writes; that objective's score does not read them
 *   cost_counts[H]       at step t the number of particles whose masked cost byte is non-zero; all -1 on CEM_VARIANT_CEM handles,
 *                        whose rollout stores no cost bytes
 *   flags                bit 0: a best-so-far update without a matching elite; never set by this library's selects
 * Launch `it` of a plan: it == 0 resets the block (sequence and returns zero, score -inf, candidate and iteration -1, counts 0 or -1,
 * flags 0) whether or not the problem is live; then, iff the select in front counted the iteration (the rule of the elite KEEP) and
 * best_score > the block's score (fp32, strict: an equal score later in the plan is no update, -0.0 against +0.0 is none), the block
 * takes the lowest-indexed elite whose score equals best_score — the select's own winner: maximum score, ties to the lowest candidate
 * index.  Comparisons, word copies and integer counts only.  Sampler, rollout, reduce, select and refit launch exactly as before:
 * cem_planner_rollout_path and cem_planner_rollout_form report what they reported, cem_planner_launches_per_iteration + 1; with
 * cem_planner_set_timing on the tracker's time is part of the select time.  Whole plans (graph and eager), the stepwise calls (each
 * cem_plan_select is followed by its tracker) and batch handles serve it, with every objective, refit, noise, carry-over and
 * population setting.  The setter waits for the stream and drops the captured graph.
 *   CEM_ERR_INVALID_ARG  null handle or pointer; enable not 0 / 1
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  enabling with world_size > 1 or a communicator (`ret` is a shard; and cem_planner_comm_init on an enabled
 *                        handle), on a handle outside the one-workgroup select (select_mode 2 / 3: the rule of cem_planner_set_refit),
 *                        or with more than 128 particles
 * A failed allocation returns CEM_ERR_HIP; the handle keeps its previous setting after any of these.
 *
 * What is valid when: cem_planner_plan / cem_planner_plan_batch return as soon as the select that ends the plan has handed action,
 * score and iterations to the host — the tracker of that iteration runs BEHIND it.  Those three are valid on return; the block is
 * complete only once the stream has drained, which cem_planner_plan_readout does itself.  It copies the block of `problem` to *out and to
 * the arrays given (each may be NULL); it may be called inside a stepwise plan, and before any plan (it then reads "nothing found").
 *   CEM_ERR_STATE        the read-out is off
 *   CEM_ERR_INVALID_ARG  null handle or `out`; problem outside [0, max(max_batch, 1)) */
typedef struct { float score; int32_t candidate, iteration, flags; } cem_plan_readout_t;
int cem_planner_set_plan_readout(cem_planner_t *h, int32_t enable);
int cem_planner_get_plan_readout(const cem_planner_t *h, int32_t *enable_out);
int cem_planner_plan_readout(cem_planner_t *h, int32_t problem, cem_plan_readout_t *out,
                             float *sequence_out_host /* [H][A] or NULL */,
                             float *particle_returns_out_host /* [P] or NULL */,
                             int32_t *cost_counts_out_host /* [H] or NULL */);

/* ---------------------------------------------------------------------------------------------------------------
 * Task scorers: plan on quadratic rewards and box state constraints.  Beyond the reference, off by default.
 * cem_scorer_t says "the observation is a Safety-Gym lidar vector and the reward is progress towards the goal lidar".  With a task set,
 * the handle scores its rollouts by the task instead: every iteration launches the sampler, the handle's MODE 1 rollout kernel (the one
 * cem_unfold_sequences runs: unchanged, writing the raw state trajectory [rows][H + 1][O] into a buffer the handle owns) and ONE more
 * kernel (cem_task_score_kernel, csrc/cem_task_score.h) that turns trajectories and actions into the returns [P][N] and cost bytes
 * [H][P][N] every later stage has always read.  The scorer fields of cem_config_t are inert on such a handle.
 *
 * For one rollout row r (particle-major: r = p * N + n, candidate n = r mod N) with states s_0 .. s_H and actions a_0 .. a_{H-1}:
 *   phi(s)  = sum_f [ q_f (s_f - g_f)^2 - c_f s_f ]                   q, g, c [obs_dim]; NULL: zeros
 *   u(a)    = sum_j rho_j a_j^2                                       rho [act_dim]; NULL: zeros
 *   near(s) = R2 > 0 and sum_f goal_mask_f (s_f - g_f)^2 <= R2        R2 = fl32(goal_radius * goal_radius); goal_mask NULL: zeros
 *   viol(s) = 1 if any s_f < lo_f or s_f > hi_f, else 0               lo NULL: -inf, hi NULL: +inf; a NaN state compares false
 * and, step by step, the reference's bookkeeping (mpc_policy.py:34-37, safe_cem_mpc.py:86-93):
 *   ga = near(s_t);  r = -phi(s_{t+1}) - u(a_t) + (ga ? reward_goal : 0);  r = clip(r, -reward_clip, reward_clip)  (reward_clip <= 0: none)
 *   CEM_VARIANT_CEM:          return += r * (done ? 0 : 1);  done |= ga
 *   CEM_VARIANT_SAFE:         done |= ga;  cost byte [t] = viol(s_t) * (done ? 0 : 1);  return += r * (done ? 0 : 1)
 *   CEM_VARIANT_COST:         as SAFE with near never true: compute_mean_costs has no done mask (safe_cem_mpc.py:98-108)
 * All of it fp32, products and sums rounded separately, in the fixed order csrc/cem_task_score.h states (planner.task_objective is
 * the NumPy restatement, bit for bit).  A NaN return is stored as 0x7fc00000.
 *
 * cem_planner_set_task copies the tables (they may be freed on return), allocates the trajectory buffer (rows * (H + 1) * obs_dim * 4
 * bytes, kept until destroy) before it changes anything, waits for the stream and drops the captured graph.  NULL or kind
 * CEM_TASK_SAFETY_GYM switches the task off: the handle then launches what it launched and returns the bits it returned.  While on,
 * cem_planner_rollout_path reports generic (no lean form, no folded sampler, no floating segments) and
 * cem_planner_launches_per_iteration counts the extra launches.  Graph, eager, stepwise and timed plans (the kernel's time is part of
 * the reduce time), population schedules, caller noise tensors and every option of the setters above serve it, on all three
 * precisions and on 129 .. 256 units.
 *   CEM_ERR_INVALID_ARG  null handle; kind not 0 / 1; a NaN or infinite q / g / c / goal_mask / rho entry, goal_radius, reward_goal or
 *                        reward_clip; a NaN bound or lo_f > hi_f; goal_radius < 0
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  a batch handle, world_size > 1 or a communicator (and cem_planner_comm_init on a handle with a task); a
 *                        library built without the kernel; a trajectory buffer beyond cem_unfold_sequences' element limit
 * A failed allocation returns CEM_ERR_HIP; the handle keeps its previous setting after any of these.
 *
 * cem_planner_task_trajectories copies the buffer as the last rollout launch left it ([P * n_samples][H + 1][obs_dim]; an iteration of
 * a population schedule fills the leading P * n[it] rows) to out_dev and waits for the stream; CEM_ERR_STATE without a task.
 * cem_task_score runs the kernel alone on the caller's device arrays with the handle's task and variant: traj [n_rows][horizon + 1]
 * [obs_dim], actions [n_rows / particles][horizon][act_dim] -> ret_out [n_rows] and, on SAFE / COST handles where it is not NULL,
 * costs_out [horizon][n_rows] bytes.  CEM_ERR_STATE without a task; CEM_ERR_INVALID_ARG for n_rows not a multiple of particles. */
enum cem_task_kind { CEM_TASK_SAFETY_GYM = 0, CEM_TASK_QUADRATIC = 1 };
typedef struct {
    int32_t kind;                 /* enum cem_task_kind */
    const float *q, *g, *c, *goal_mask, *lo, *hi;   /* [obs_dim] each, host memory, or NULL for the default */
    const float *rho;             /* [act_dim], host memory, or NULL */
    float goal_radius, reward_goal, reward_clip;
} cem_task_t;
int cem_planner_set_task(cem_planner_t *h, const cem_task_t *task);
int cem_planner_task_trajectories(cem_planner_t *h, float *out_dev);
int cem_task_score(cem_planner_t *h, const float *traj_dev, const float *actions_dev, int32_t n_rows, int32_t horizon,
                   float *ret_out_dev, uint8_t *costs_out_dev);

/* ---------------------------------------------------------------------------------------------------------------
 * Tracking tasks: a per-step reference, terminal weights and an action-rate penalty.  Beyond the reference, off by default (DESIGN.md
 * 4.20).  A second task kind: the quadratic task above with row j of a reference table ref [ref_steps][obs_dim] in the place of g for the
 * state that lies j - k0 steps into the plan, a weight vector of its own on the last predicted state, and a penalty on the change of the
 * action from one step to the next.  The handle keeps a "clock" (k0, previous action) in device memory; cem_planner_set_task_clock moves
 * it between decisions with a stream-ordered copy, so the captured graph stays.  A tracking plan launches what a quadratic-task plan
 * launches, with the kernel of csrc/cem_task_reference.h, cem_task_reference_kernel, in the place of cem_task_score_kernel.
 *
 * Everything not named here is the quadratic task's, statement for statement.  q, c, goal_mask, lo, hi, rho, goal_radius, reward_goal,
 * reward_clip come from `base` (base->kind CEM_TASK_QUADRATIC, base->g NULL); q_terminal [obs_dim] defaults to q, action_rate
 * [act_dim] (kappa) to zeros.  For state s_st, st = 0 .. H:
 *   j = min(k0 + st, ref_steps - 1)                                     the last row is held
 *   phi(s_st)  = sum_f [ w_f (s_f - ref[j]_f)^2 - c_f s_f ]             w = q_terminal where st == H, else q
 *   near(s_st) = R2 > 0 and sum_f goal_mask_f (s_f - ref[j]_f)^2 <= R2
 *   v_t = sum_j kappa_j (a_t[j] - a_{t-1}[j])^2                          a_{-1}: the clock's previous action
 *   r   = -phi(s_{t+1}) - u(a_t) - v_t + (near(s_t) ? reward_goal : 0)   then the clip and the variant's bookkeeping as above
 * in fp32, every product, difference and sum rounded on its own, in the order csrc/cem_task_reference.h states
 * (planner.tracking_objective is the NumPy restatement, bit for bit).  With ref_steps = 1, ref[0] = g and neither q_terminal nor
 * action_rate the returns and cost bytes are the quadratic task's, bit for bit.
 *
 * cem_planner_set_task_tracking copies the tables (they may be freed on return), allocates the reference table (ref_steps rows of 512
 * bytes), the clock block and, where the handle has none yet, the trajectory buffer before it changes anything, waits for the stream and
 * drops the captured graph, as cem_planner_set_task does; the clock resets to (0, zeros).  cem_planner_set_task(h, NULL) switches
 * either kind off; cem_planner_set_task itself accepts kinds 0 and 1 only.  cem_planner_task_trajectories and cem_task_score serve both
 * kinds; cem_task_score scores with the handle's clock.
 *   CEM_ERR_INVALID_ARG  null handle, base or trk; base->kind not CEM_TASK_QUADRATIC; base->g not NULL; ref NULL; ref_steps < 1 or
 *                        > CEM_TASK_REF_MAX_STEPS; a NaN or infinite ref, q_terminal or action_rate entry; whatever cem_planner_set_task
 *                        refuses in base
 *   CEM_ERR_STATE        between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  what cem_planner_set_task refuses so; a library built without cem_task_reference_kernel
 * A failed allocation returns CEM_ERR_HIP; the handle keeps its previous setting after any of these.
 *
 * cem_planner_set_task_clock sets k0 and, unless prev_action is NULL, the previous action [act_dim] (host memory, copied before the call
 * returns).  A stream-ordered copy, as cem_planner_set_cost_budget's: plans enqueued later see it, nothing waits, the captured graph and
 * its node count stay.
 *   CEM_ERR_INVALID_ARG  null handle; k0 < 0; a NaN or infinite prev_action entry
 *   CEM_ERR_STATE        no tracking task in force; between the begin and end calls of a stepwise plan */
#define CEM_TASK_REF_MAX_STEPS 16384
enum cem_task_kind_more { CEM_TASK_TRACKING = 2 };   /* a third value for the kind fields, which hold an int32_t */
typedef struct {
    const float *ref;             /* [ref_steps][obs_dim], host memory */
    int32_t ref_steps;            /* 1 .. CEM_TASK_REF_MAX_STEPS */
    const float *q_terminal;      /* [obs_dim], host memory, or NULL: base->q */
    const float *action_rate;     /* [act_dim], host memory, or NULL: zeros */
} cem_task_tracking_t;
int cem_planner_set_task_tracking(cem_planner_t *h, const cem_task_t *base, const cem_task_tracking_t *trk);
int cem_planner_set_task_clock(cem_planner_t *h, int32_t k0, const float *prev_action /* [act_dim] or NULL: unchanged */);

/* ---------------------------------------------------------------------------------------------------------------
 * Zones: keep-out and keep-in regions on a task.  Beyond the reference, off by default.  A task of either kind may
 * carry up to CEM_TASK_MAX_ZONES zones: axis-aligned ellipsoids on up to CEM_TASK_ZONE_AXES state features each — discs, spheres,
 * cylinders (features left out) — which the state must stay out of, or with keep_in inside of.  A state that hits a zone is a violation
 * exactly as a state outside the box is; a state within `margin` of a zone pays `penalty` times a hinge.  A plan with zones launches what
 * its base task plan launches, with the kernel of csrc/cem_task_zones.h, cem_task_zones_kernel, in the place of cem_task_score_kernel /
 * cem_task_reference_kernel.  A task without zones launches what it launched and returns the bits it returned.
 *
 * Zone z: axis[z][d], d = 0 .. 3, a feature index or -1 (slot unused; at least one used), centre[z][d], weight[z][d] >= 0, radius[z] > 0,
 * margin[z] >= 0, penalty[z] >= 0, keep_in[z] 0 / 1.  In fp32, every product, difference and sum rounded on its own:
 *   dist2_z(s) starts at +0; for d = 0 .. 3 with a used axis:  e = s[axis] - centre;  dist2 = dist2 + weight * (e * e)
 *   R2_z = fl32(radius * radius);  Rm2_z = fl32((radius + margin) * (radius + margin)), keep-in: fl32((radius - margin) * (radius - margin))
 *   with margin <= radius; both rounded once by this call
 *   keep-out:  hit_z = dist2 <= R2;  hinge_z = fmaxf(Rm2 - dist2, 0)          keep-in:  hit_z = dist2 > R2;  hinge_z = fmaxf(dist2 - Rm2, 0)
 *   a NaN dist2 hits nothing and its hinge is 0
 *   pen(s): sixteen slots, slot z = penalty_z * hinge_z, slots from n_zones on +0, added pairwise, neighbours first, over four levels
 *   viol(s) = the box's viol(s) or any hit_z(s): the cost of step t is viol(s_t) * nd as before, in every variant
 *   r = -phi(s_{t+1}) - u(a_t) - v_t - pen(s_{t+1}) + (near(s_t) ? reward_goal : 0), in that order; then the clip as before
 * (v_t: a tracking task's action-rate term; a quadratic task has none).  planner.task_objective / tracking_objective restate it, bit for
 * bit.  Zones that are never hit and have penalty 0 leave every result bit of the base task.
 *
 * cem_planner_set_task_zones copies the tables (they may be freed on return), allocates before it changes anything, waits for the
 * stream and drops the captured graph, as cem_planner_set_task does.  zones NULL clears them (and is a no-op on a handle without any).
 * cem_planner_set_task and cem_planner_set_task_tracking clear them too: set the task, then its zones.  cem_planner_set_task_clock,
 * cem_planner_task_trajectories and cem_task_score serve a plan with zones as they serve its base task.
 *   CEM_ERR_INVALID_ARG  null handle; n_zones outside 1 .. CEM_TASK_MAX_ZONES; axis, centre, weight or radius NULL; an axis < -1 or
 *                        >= obs_dim; a zone without a used axis; a NaN or infinite entry; a weight, margin or penalty below 0; a
 *                        radius <= 0; keep-in with margin > radius; a keep_in entry that is not 0 or 1
 *   CEM_ERR_STATE        no task in force; between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  a library built without cem_task_zones_kernel
 * A failed allocation returns CEM_ERR_HIP; the handle keeps its previous setting after any of these. */
#define CEM_TASK_MAX_ZONES 16
#define CEM_TASK_ZONE_AXES 4
typedef struct {
    int32_t n_zones;              /* 1 .. CEM_TASK_MAX_ZONES */
    const int32_t *axis;          /* [n_zones][CEM_TASK_ZONE_AXES], host memory: feature indices, -1: unused */
    const float *centre;          /* [n_zones][CEM_TASK_ZONE_AXES] (an unused slot's entry is not read) */
    const float *weight;          /* [n_zones][CEM_TASK_ZONE_AXES] (an unused slot's entry is not read) */
    const float *radius;          /* [n_zones] */
    const float *margin;          /* [n_zones], or NULL: zeros */
    const float *penalty;         /* [n_zones], or NULL: zeros */
    const int32_t *keep_in;       /* [n_zones], or NULL: zeros (keep-out) */
} cem_task_zones_t;
int cem_planner_set_task_zones(cem_planner_t *h, const cem_task_zones_t *zones /* NULL: none */);

/* ---------------------------------------------------------------------------------------------------------------
 * Linear outputs: derived features y = C s on a task.  Beyond the reference, off by default.  A task of either kind
 * may carry M = n_outputs <= CEM_TASK_MAX_OUTPUTS linear outputs of the state, and each output has the task's whole vocabulary: a
 * weight, a target (or a per-step reference on a tracking base), a linear term, a near-goal weight, a box bound, a terminal weight,
 * and a zone may name it as an axis by the index obs_dim + m.  With Q = L^T L the full-matrix cost (x - x_ref)^T Q (x - x_ref) is
 * matrix = L, weight = 1, target = L x_ref; a bound hi on an output is the half-space C[m] . s <= hi, M of them a polytope; two
 * outputs under a rotation carry a rotated ellipse.  A plan with outputs launches what its base task plan launches, with the kernel
 * of csrc/cem_task_outputs.h, cem_task_outputs_kernel, in the place of the task's (or the zones') kernel.  A task without outputs
 * launches what it launched and returns the bits it returned.
 *
 * In fp32, every product, difference and sum rounded on its own, for state s and output m:
 *   y_m(s): sixteen partial sums; partial l starts at +0 and adds matrix[m][f] * s_f for f = 64 i + 4 l + r, i = 0, 1 and then
 *           r = 0 .. 3 (features >= obs_dim add nothing); the sixteen are added pairwise, neighbours first, over four levels
 *   e = y_m - target_m   (a tracking base with ref_rows = T: row min(k0 + st, T - 1) of `reference`, the base task's clock);  ee = e * e
 *   w = weight_m, on the terminal state of a tracking base terminal_m (NULL: weight)
 *   phi(s): partial m of its sixteen also adds (w * ee - linear_m * y_m), behind that partial's features;  near's partial m adds near_m * ee
 *   viol(s) also holds where some y_m < lo_m or y_m > hi_m (a NaN compares false)
 *   a zone axis obs_dim + m reads y_m where a feature axis reads s[axis]
 * Everything else is the zones' contract above.  planner.output_terms, task_objective and tracking_objective restate it, bit for bit.
 * Outputs with weight = linear = near = terminal = 0 and infinite bounds leave every result bit of the task without them.
 *
 * cem_planner_set_task_outputs copies the tables (they may be freed on return), allocates before it changes anything, waits for the
 * stream and drops the captured graph, as cem_planner_set_task_zones does.  outputs NULL clears them (a no-op on a handle without any).
 * The call clears the zones; cem_planner_set_task and cem_planner_set_task_tracking clear the outputs: set the task, then its
 * outputs, then its zones.  While outputs are in force cem_planner_set_task_zones accepts axes in [obs_dim, obs_dim + n_outputs).
 * cem_planner_set_task_clock, cem_planner_task_trajectories and cem_task_score serve a plan with outputs as they serve its base task.
 *   CEM_ERR_INVALID_ARG  null handle; n_outputs outside 1 .. CEM_TASK_MAX_OUTPUTS; matrix NULL; a NaN or infinite matrix, weight,
 *                        target, linear, near or terminal entry; a weight or terminal below 0; a NaN bound or lo > hi; ref_rows that
 *                        is neither 1 nor the base task's ref_steps (a quadratic base: 1; 0 with reference NULL counts as 1)
 *   CEM_ERR_STATE        no task in force; between the begin and end calls of a stepwise plan
 *   CEM_ERR_UNSUPPORTED  a library built without cem_task_outputs_kernel
 * A failed allocation returns CEM_ERR_HIP; the handle keeps its previous setting after any of these. */
#define CEM_TASK_MAX_OUTPUTS 16
typedef struct {
    int32_t n_outputs;            /* 1 .. CEM_TASK_MAX_OUTPUTS */
    const float *matrix;          /* [n_outputs][obs_dim], host memory */
    const float *weight;          /* [n_outputs], or NULL: zeros */
    const float *target;          /* [n_outputs], or NULL: zeros; not read where `reference` is given */
    const float *linear;          /* [n_outputs], or NULL: zeros */
    const float *near;            /* [n_outputs], or NULL: zeros */
    const float *lo;              /* [n_outputs], or NULL: -inf */
    const float *hi;              /* [n_outputs], or NULL: +inf */
    const float *terminal;        /* [n_outputs], or NULL: weight */
    int32_t ref_rows;             /* rows of `reference`: 1 or the base task's ref_steps */
    const float *reference;       /* [ref_rows][n_outputs], or NULL: `target` on every step */
} cem_task_outputs_t;
int cem_planner_set_task_outputs(cem_planner_t *h, const cem_task_outputs_t *outputs /* NULL: none */);

/* ---------------------------------------------------------------------------------------------------------------
 * Ensemble training on the device: MlpEnsemble.training_step / validation_step
 * (simba/models/mlp_ensemble.py:134-155), loss negative_log_likelihood (:64-67), optimizer
 * tf.keras.optimizers.Adam(lr, clipvalue=1.0, epsilon=1e-5) (:113-117).  The shuffling / batching / learning-rate
 * schedule loop of fit() (:163-187, :70-88) is host logic above this ABI.  Weights use the natural blob layout above,
 * so the result of training feeds cem_planner_set_weights() unchanged.
 * A step takes 1 .. batch_size <= CEM_TRAIN_MAX_BATCH rows per member; a larger batch_size is CEM_ERR_UNSUPPORTED (and a workspace
 * size of 0).  Each member's rows are split into at most 32 row parts (one workgroup each), which take their rows in passes of 16
 * and leave partial gradients that the Adam step adds in part order: no atomics, repeated steps give identical bits.  Up to 64 rows
 * every part is one pass of 16 rows.  validation_step walks the set in chunks of min(batch_size, 64) rows. */
#define CEM_TRAIN_MAX_BATCH 4096
typedef struct cem_train_config {
    int32_t abi_version;
    int32_t inputs_dim, outputs_dim, units, n_layers, ensemble_size;
    int32_t batch_size;           /* rows per member per step, 1 .. CEM_TRAIN_MAX_BATCH (config/models.yaml:4 ships 64) */
    int32_t activation;           /* enum cem_activation */
    float dropout_rate;           /* mlp_params['dropout_rate'] (config/models.yaml:13; the shipped value is 0): Dropout after every hidden layer in
                                   * training_step only (mlp_ensemble.py:15,21,138); 0 <= rate < 1.  The keep mask of training step s (0-based,
                                   * counted from cem_trainer_create — cem_trainer_set_state does not restart it, so re-staged weights do not replay masks) is a pure function of (dropout_seed, s, member,
                                   * layer, row of the minibatch, unit): cem_train.h GemmEpi */
    uint32_t dropout_seed_lo, dropout_seed_hi;
    float beta1, beta2, epsilon, clipvalue;      /* Adam: 0 <= beta < 1; epsilon and clipvalue finite and > 0 (anything else is CEM_ERR_INVALID_ARG
                                   * and a workspace size of 0).  Every gradient element — the sum over the row parts — is clipped to
                                   * +-clipvalue; for "no clip" pass a large finite value such as 1e30 (infinity is refused) */
} cem_train_config_t;
typedef struct cem_trainer cem_trainer_t;

size_t cem_trainer_workspace_bytes(const cem_train_config_t *cfg);
size_t cem_trainer_blob_floats(const cem_train_config_t *cfg);
int cem_trainer_create(const cem_train_config_t *cfg, void *workspace, size_t workspace_bytes, void *hip_stream, cem_trainer_t **out);
int cem_trainer_destroy(cem_trainer_t *h);
/* weights + Adam moments (host blobs; moments may be NULL = zeros) */
int cem_trainer_set_state(cem_trainer_t *h, const float *weights, const float *m, const float *v);
int cem_trainer_get_state(cem_trainer_t *h, float *weights, float *m, float *v);
/* the trainer's current weights where they live: a device pointer into its workspace (valid until destroy; contents follow the
 * trainer's stream) and the float count — what cem_planner_set_weights_dev takes */
int cem_trainer_weights_dev(cem_trainer_t *h, const float **blob_dev_out, size_t *n_floats_out);
/* one training_step on rows perm[member][offset .. offset+bt) of x_dev[n][inputs_dim] / y_dev[n][outputs_dim];
 * lr_t = lr * sqrt(1-beta2^t)/(1-beta1^t) (Keras folds the bias correction into the step size);
 * loss_dev[ensemble_size] receives every member's share of the loss (their sum is training_step's return value) */
int cem_trainer_step(cem_trainer_t *h, const float *x_dev, const float *y_dev, const int32_t *perm_dev, int32_t nperm,
                     int32_t offset, int32_t bt, float lr_t, float *loss_dev);
/* n_steps consecutive training_steps in ONE call (an epoch of MlpEnsemble.fit's inner loop, mlp_ensemble.py:174-180): step s uses
 * rows perm[member][offsets[s] .. offsets[s] + bts[s]) with step size lr_ts[s] (host arrays) and writes its members' losses to
 * loss_dev[s * ensemble_size ..].  Same arithmetic as n_steps cem_trainer_step calls; the point is one host call per epoch. */
int cem_trainer_steps(cem_trainer_t *h, const float *x_dev, const float *y_dev, const int32_t *perm_dev, int32_t nperm,
                      int32_t n_steps, const int32_t *offsets, const int32_t *bts, const float *lr_ts, float *loss_dev);
/* validation_step on rows [0, n) of x_dev / y_dev: *loss_out = sum over members of NLL / ensemble_size (synchronises) */
int cem_trainer_eval(cem_trainer_t *h, const float *x_dev, const float *y_dev, int32_t n, float *loss_out);

/* Ensemble inference on the trainer's weights: MlpEnsemble.forward (mlp_ensemble.py:122-132: tf.split of the batch over the members,
 * mu and var concatenated back) and MlpEnsemble.__call__ (:189-193: Normal(mu, sqrt(var)) -> mean, stddev, sample), and with
 * CEM_FORWARD_ALL the member x row map of validation_step (:150-154: every member on the same rows).
 * x_dev[n_rows][inputs_dim] holds inputs that are already scaled; nothing is normalised and no state is added.
 *   CEM_FORWARD_SPLIT  n_rows must be a multiple of ensemble_size (else CEM_ERR_SPLIT, as tf.split raises); row r is evaluated by member
 *                      r / (n_rows / ensemble_size); outputs are [n_rows][outputs_dim]
 *   CEM_FORWARD_ALL    every member evaluates every row; outputs are [ensemble_size][n_rows][outputs_dim]
 * Outputs (device pointers, each may be NULL = not written; all four NULL is CEM_ERR_INVALID_ARG): mu; var = softplus(v) + 1e-4, the value
 * training_step's loss sees; sd = sqrt(var); sample = mu + sd * eps with one rounding per operation.  eps_dev: standard normals in the
 * sample's shape, or NULL for Philox noise at the counters documented for cem_philox_words: stream 0, idx = output row (SPLIT: r, ALL:
 * member * n_rows + r), t = iteration = 0, sub = feature quad, key from (seed, call).  No noise is drawn when sample_out_dev is NULL.
 * Stream-ordered on the trainer's stream like cem_trainer_steps (no synchronisation); reads the weights only: the Adam moments and the
 * step counter are untouched.  CEM_ERR_INVALID_ARG for a NULL handle or x_dev, n_rows < 1 or an unknown map; CEM_ERR_UNSUPPORTED for
 * ensemble_size x rows per member >= 2^32. */
enum cem_forward_map { CEM_FORWARD_SPLIT = 0, CEM_FORWARD_ALL = 1 };
int cem_trainer_forward(cem_trainer_t *h, const float *x_dev, int32_t n_rows, int32_t map, const float *eps_dev, uint64_t seed, uint64_t call,
                        float *mu_out_dev, float *var_out_dev, float *sd_out_dev, float *sample_out_dev);

#ifdef __cplusplus
}
#endif
#endif /* CEM_MPC_H */
