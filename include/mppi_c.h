/*
 * mppi_c.h — C-ABI of the MI355X-native MPPI control step (libmppi_hip.so).
 *
 * This is the drop-in boundary for ONE path of NicolayP/mppi-tf: the per-control-step MPPI
 * update (perturb K control sequences, roll the model H steps, cost every step, soft-min
 * weight, reduce to the new nominal sequence).  The reference has no FFI of its own; its
 * boundary is the public C++ API of `ControllerBase` (include/controller_base.hpp:60-109 in
 * the reference) as driven by its host loop (src/main.cpp:30-45).  Every entry point below
 * names the reference interface it replaces.  include/mppi/controller_base.hpp re-creates
 * the reference's C++ classes on top of these calls; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - plain C, no torch / HIP types in signatures; `void *stream` is a hipStream_t (NULL = the
 *    handle's own, non-blocking stream; to enqueue on the legacy default stream — torch's default — pass
 *    hipStreamLegacy, (hipStream_t)1: a step must run on a stream that is ordered against whatever produces
 *    x_dev and consumes u_dev / the records);
 *  - all host buffers are caller-owned, fp32, row-major, with the reference's trailing
 *    singleton dropped:  x[s]  U[tau,a]  eps[K,tau,a]  cost[K];
 *  - pointers named *_dev are DEVICE pointers on the handle's GPU;
 *  - every call returns an mppi_status (0 = OK) and never aborts (the reference LOG(FATAL)s
 *    on a TF error, controller_base.cpp:141); mppi_last_error() gives the text;
 *  - one handle = one controller, NOT thread-safe per handle (same as the reference: one
 *    session, mutable m_U); distinct handles are independent;
 *  - host-pointer calls are synchronous; *_device calls only enqueue on the stream.
 */
#ifndef MPPI_C_H_
#define MPPI_C_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPI_ABI_VERSION 5 /* 5: MPPI_TUNE_FUSED_STEP / _ARMED_US / _ARMED_ALWAYS / _PRELAUNCH (no entry point changed), mppi_run_episode / mppi_batch_run_episode
                              (added; no entry point changed), mppi_learner_gradients and the [in, 256, 256, out] learner (added; no entry point changed),
                              mppi_learner_batch_* (added; no entry point changed), mppi_create_batch_learned / mppi_batch_set_mlp (added; no entry point changed),
                              mppi_learner_wide_batch_* (added; no entry point changed), mppi_create_batch_mlp (added; no entry point changed);
                              4: mppi_shard_step (one call per sharded step, the caller's collectives as function pointers), mppi_learner_save /
                              _load / _peek, MPPI_TUNE_TRACE (roctx ranges); mppi_set_mlp orders against the last step's stream;
                              3: the 13-state AUV family (MPPI_MODEL_AUV / _NN_AUV, mppi_auv_desc), StaticQuatCost / ElipseCost3D state costs,
                              mppi_auv_pieces, the learner (mppi_learner_*); 2: state_cost_kind / ellipse, transition log, tuning */
#define MPPI_MAX_S 32  /* largest state dimension  */
#define MPPI_MAX_A 16  /* largest action dimension */

typedef struct mppi_handle mppi_handle;

typedef enum {
    MPPI_OK = 0,
    MPPI_ERR_INVALID_ARG = 1,    /* bad size / NULL (ref: setGoal -> false, controller_base.cpp:126-130) */
    MPPI_ERR_NO_DEVICE = 2,      /* no HIP device / device ordinal out of range */
    MPPI_ERR_HIP = 3,            /* a HIP runtime call failed; see mppi_last_error */
    MPPI_ERR_UNSUPPORTED = 4,    /* shape / option outside what the kernels implement */
    MPPI_ERR_SINGULAR_SIGMA = 5, /* Σ not invertible (ref: MatrixInverse fails, cost_base.cpp:39) */
    MPPI_ERR_ALLOC = 6,
    MPPI_ERR_IO = 7,
    MPPI_ERR_EXCHANGE = 8        /* direct record exchange: a packet missed its deadline (mppi_shard_p2p_step) */
} mppi_status;

enum { MPPI_MODEL_POINT_MASS = 0, /* x' = A x + (B/m) v, src/model_base.cpp:53-82 */
       MPPI_MODEL_MLP = 1,        /* x' = x + denorm(MLP(norm([x;v]))), nn_model.py:215-304 convention, point-mass state (s = 2a) */
       MPPI_MODEL_AUV = 2,        /* Fossen 6-DOF AUVModel, s = 13 (pos, quat xyzw, lin vel, ang vel), a = 6: models/auv_model.py:282-562 */
       MPPI_MODEL_NN_AUV = 3,     /* NNAUVModel: x' = x + denorm(nn(norm(concat(x[3:], u)))), s = 13, a = 6, nn input s+a-3 = 16,
                                     Dense(16|32, relu) x 1..3 + Dense(13): models/nn_model.py:179-304 */
       MPPI_MODEL_NN_AUV_SPEED = 4 }; /* NNAUVModelSpeed: the network predicts the velocity delta from (Euler angles, velocities,
                                     forces) = 15 inputs, Dense(16|32, relu) x 1..3 + Dense(6); the pose is integrated with the
                                     quaternion kinematics over cfg.dt and renormalised: models/nn_model.py:307-588 */

enum { MPPI_ACTION_COST_CPP = 0,  /* λ uᵀΣ⁻¹ε                          src/cost_base.cpp:63-68   */
       MPPI_ACTION_COST_PY = 1 }; /* ½[γ(uᵀΣ⁻¹u+2uᵀΣ⁻¹ε)+λ(1-1/υ)εᵀΣ⁻¹ε]  costs/cost_base.py:114-170 */

enum { MPPI_STATE_COST_QUADRATIC = 0, /* (x-g)ᵀQ(x-g)   src/cost_base.cpp:56-61, costs/static_cost.py:40-63          */
       MPPI_STATE_COST_ELLIPSE = 1,   /* 2D elliptic track, state (x, vx, y, vy, ..): m_state·|((x-cx)/a)²+((y-cy)/b)²-1|
                                         + m_vel·(sqrt(vx²+vy²)-speed)²                 costs/elipse_cost.py:9-85       */
       MPPI_STATE_COST_QUAT = 2,      /* StaticQuatCost (s = 13): d = (pos-g, 2·acos<quat, g_quat>, vel-g) [10], dᵀ Q d with
                                         Q = cfg.quat_Q [10*10], goal = cfg.goal [13]      costs/static_cost.py:73-159  */
       MPPI_STATE_COST_ELLIPSE3D = 3 };/* ElipseCost3D (s = 13): the pose taken into the ellipse's plane frame, then
                                         mS·|Σ(p_i/axis_i)²-1| + mS·angle(pose, tangent) + mV·||v|²-speed²|
                                         with cfg.ellipse3d                                costs/elipse_cost.py:101-246 */

/* mppi_config.flags */
enum { MPPI_FLAG_UPSILON_SCALES_NOISE = 1, /* Py build_noise: eps = (υΣ)·z while the cost keeps Σ⁻¹ of the
                                              un-augmented Σ (controller_base.py:362-368, cost_base.py:35-41) */
       MPPI_FLAG_MLP_BF16X3 = 2, /* learned models (point mass: 256- or 32-wide hidden layers; NNAUVModel: 32-wide): the layers run on the BF16
                                   matrix cores with every fp32 operand split into two bf16 values and three products per
                                   term (fp32 accumulate): ~2x the rounding error of the exact-fp32 path (sample costs
                                   within 1e-6 relative of fp64 on the synthetic network), 1.7-3.3x its speed. Off by
                                   default: the default MLP path is exact fp32 (v_mfma_f32_32x32x2_f32). */
       MPPI_FLAG_FP_CONTRACT = 4 /* point mass, diagonal quadratic cost, Philox noise: the rollout kernel evaluates the model step, the state cost
                                   and the action cost with FUSED multiply-adds (one rounding per pair instead of two) — ~15 % fewer vector
                                   instructions in an issue-bound kernel. Sample costs are then NOT bit-identical to the reference's op-by-op
                                   fp32 evaluation: they agree with an fp64 evaluation to 2e-6 relative (as the unfused evaluation does), the update to 1e-5 (tests). Off by
                                   default; the fused one-launch step and the armed launches are not taken by such a handle. */ };

/* what mppi_debug_get returns (observer_base.py:101-187 logs the same intermediates) */
enum { MPPI_DBG_COSTS = 0,    /* c[K_local]         sample costs of the last step            */
       MPPI_DBG_BETA = 1,     /* [1]                min cost (over all shards after finish)  */
       MPPI_DBG_ETA = 2,      /* [1]                Σ exp(-(c-β)/λ)                          */
       MPPI_DBG_WEIGHTS = 3,  /* w[K_local]         exp(-(c-β)/λ)/η                          */
       MPPI_DBG_NOISE = 4,    /* eps[K_local,tau,a] the noise the last step used             */
       MPPI_DBG_U_UPDATED = 5,/* U'[tau,a]          updated sequence before the shift        */
       MPPI_DBG_AUX = 6       /* [8]                beta, eta, and the words timing-study builds stamp (tools/timeline_step.py) */ };

/* Learned model_base: Dense(relu) x (n_layers-1) + Dense(linear) -> s_dim outputs. */
typedef struct {
    int32_t n_layers;
    const int32_t *widths;   /* [n_layers] output width of every layer; widths[n_layers-1] == s_dim */
    const float *const *W;   /* W[l]: [in x out] row-major (Keras kernel layout)                    */
    const float *const *b;   /* b[l]: [out]                                                         */
    const float *xmean, *xstd; /* [s+a] input normalisation, NULL -> 0 / 1 (nn_model.py:289-293)     */
    const float *ymean, *ystd; /* [s]   output de-normalisation, NULL -> 0 / 1 (nn_model.py:295-297) */
} mppi_mlp_desc;

/* AUVModel's `parameters` (models/auv_model.py:85-245; config/models/rexrov2.default.yaml). Matrices [6*6] row-major; a
 * diagonal given in the reference's 6-vector form is expanded by the caller. NULL matrix = zeros. */
typedef struct {
    float mass, volume, density;
    float gravity;             /* 0 -> 9.81 (auv_model.py:236) */
    float cog[3], cob[3];      /* centre of gravity / buoyancy in the body frame */
    float inertial[6];         /* ixx, iyy, izz, ixy, ixz, iyz */
    const float *added_mass;                    /* Ma [36] */
    const float *linear_damping;                /* [36] */
    const float *linear_damping_forward_speed;  /* [36] */
    const float *quad_damping;                  /* [6]  */
    int32_t rk;                /* 1 Euler, 2 Heun, 4 the reference's rk4 expression (auv_model.py:282-306) */
} mppi_auv_desc;

/* Everything the reference hard-codes in ControllerBase's constructor
 * (controller_base.cpp:23-71) or reads from its config YAML files, as one POD block. */
typedef struct {
    uint32_t struct_size;     /* = sizeof(mppi_config); set by mppi_config_init */
    int32_t k;                /* samples K (GLOBAL count when sharded)          */
    int32_t tau;              /* horizon H                                      */
    int32_t s_dim, a_dim;
    float dt, mass;
    float lambda, gamma, upsilon;
    int32_t action_cost_kind; /* MPPI_ACTION_COST_*                             */
    int32_t normalize_cost;   /* Py normalizeCost, controller_base.py:468-474   */
    const float *sigma;       /* [a*a] Σ multiplies z AND Σ⁻¹ enters the cost; NULL -> I  */
    const float *goal;        /* [s]; NULL -> (1,0) per axis (controller_base.cpp:43-46)  */
    const float *Q;           /* NULL -> ones (controller_base.cpp:58-60)                 */
    int32_t q_is_full;        /* 0: Q is the [s] diagonal (C++ Diag(in_Q)); 1: Q is [s*s] (Py) */
    uint64_t seed;            /* Philox key; default 1 (controller_base.cpp:199)          */
    int32_t model_kind;       /* MPPI_MODEL_*                                             */
    const mppi_mlp_desc *mlp; /* only for MPPI_MODEL_MLP                                  */
    int32_t device;           /* HIP device ordinal                                       */
    int32_t shard_rank;       /* this handle owns samples [rank*k/count, (rank+1)*k/count) */
    int32_t shard_count;      /* 1 = unsharded                                            */
    int32_t flags;            /* MPPI_FLAG_* bits, 0 = the C++ reference's behaviour      */
    int32_t state_cost_kind;  /* MPPI_STATE_COST_*; 0 = the quadratic cost (goal, Q)       */
    const float *ellipse;     /* MPPI_STATE_COST_ELLIPSE: [7] a, b, cx, cy, speed, m_state, m_vel (ElipseCost's
                                 constructor arguments, elipse_cost.py:10-46); needs s_dim >= 4 */
    const mppi_auv_desc *auv; /* MPPI_MODEL_AUV only */
    const float *quat_Q;      /* MPPI_STATE_COST_QUAT: Q [10*10] row-major (static_cost.py:92-100) */
    const float *ellipse3d;   /* MPPI_STATE_COST_ELLIPSE3D: [11] normal[3], aVec[3], axis a, b, speed, mState, mVel
                                 (ElipseCost3D's constructor arguments, elipse_cost.py:102-140; `center` is stored by the
                                 reference and never used) */
} mppi_config;

/* ---- library ------------------------------------------------------------------------- */
int mppi_abi_version(void);
const char *mppi_version(void);
const char *mppi_status_string(mppi_status st);
/* number of visible HIP devices (0 when there is none; never fails) */
int mppi_device_count(void);

/* ---- construction (replaces ControllerBase::ControllerBase, controller_base.cpp:23-71) -- */
/* Fill cfg with the reference constructor's defaults: λ=1, γ=υ=1, Σ=I, Q=1, goal=(1,0)…,
 * seed=1, point-mass model, C++ action cost, device 0, unsharded. */
mppi_status mppi_config_init(mppi_config *cfg, int k, int tau, float dt, float mass, int s_dim, int a_dim);
/* Build the controller: copies every array in cfg, allocates device state (U = 0). */
mppi_status mppi_create(const mppi_config *cfg, mppi_handle **out);
/* replaces ControllerBase::~ControllerBase (controller_base.cpp:124) */
void mppi_destroy(mppi_handle *h);
const char *mppi_last_error(const mppi_handle *h);

/* ---- the host loop's calls -------------------------------------------------------------- */
/* replaces ControllerBase::setGoal (controller_base.cpp:126-133). Takes effect on the next
 * step (the reference bakes the goal into the graph and ignores later calls — a bug we do
 * not reproduce). n must equal s_dim. */
mppi_status mppi_set_goal(mppi_handle *h, const float *goal, int n);
/* Replaces the learned model's weights and normalisation on an existing handle (same layer widths as at creation): what the
 * reference's learner does to the variables the controller's graph reads (learners/learner_base.py:469-496 apply_gradients;
 * models/nn_model.py set_Xmean_Xstd / set_Ymean_Ystd / update_weights). Waits for the handle's stream AND for the stream the last
 * device-resident step was enqueued on (mppi_next_device / mppi_shard_*: a rollout in flight must not read half-replaced weights;
 * ADVICE r03), copies, takes effect with the next step. MPPI_MODEL_MLP / _NN_AUV / _NN_AUV_SPEED handles. */
mppi_status mppi_set_mlp(mppi_handle *h, const mppi_mlp_desc *mlp);
/* replaces ControllerBase::next (controller_base.cpp:135-153): one control step with noise
 * drawn on the device (Philox4x32-10 via rocRAND's engine); returns u = U'[0] in u_out[a],
 * keeps shift(U') as the warm start, logs (x,u) like m_db.addX/addU. */
mppi_status mppi_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u);
/* Same step with the noise INJECTED (the reference's tests inject noise,
 * test_controller.cpp:24-35): eps is [K_local, tau, a] for this handle's shard. */
mppi_status mppi_next_with_noise(mppi_handle *h, const float *x, int n_x, const float *eps, size_t n_eps,
                                 float *u_out, int n_u);
/* The transition log (m_db, data_base.cpp:14-71). The reference appends to it on every next(); here it is a
 * preallocated ring of max_rows rows that must be switched on (the C++ / Python ControllerBase mirrors do so in their
 * constructors): 0 = off (default, nothing is recorded and mppi_next allocates nothing). Clears the log. When full
 * the oldest row is overwritten. */
mppi_status mppi_set_transition_log(mppi_handle *h, int max_rows);
/* What mppi_to_csv will NOT write, so that a truncated file never goes unnoticed (the reference's m_db grows without bound and
 * writes every transition, data_base.cpp:52-71): rows_overwritten = transitions lost because the ring was full since the log
 * was sized; rows_without_successor = rows held whose saveNext was skipped (left out of the CSV). Any output may be NULL. */
mppi_status mppi_transition_log_stats(mppi_handle *h, uint64_t *rows_held, uint64_t *rows_overwritten, uint64_t *rows_without_successor);
/* replaces ControllerBase::saveNext (controller_base.cpp:155-163): x_next is the successor of the LAST logged (x, u);
 * a row whose saveNext was skipped is left out of the CSV instead of shifting the later rows. */
mppi_status mppi_save_next(mppi_handle *h, const float *x_next, int n);
/* replaces ControllerBase::toCSV -> DataBase::toCSV (controller_base.cpp:164, data_base.cpp:52-71), byte for byte:
 * header cells and values each followed by ',' (lines end with a comma), values as std::to_string(float) = "%f". */
mppi_status mppi_to_csv(mppi_handle *h, const char *filename);
enum { MPPI_CSV_REFERENCE = 0,  /* the reference's bytes (see mppi_to_csv)                     */
       MPPI_CSV_ROUNDTRIP = 1 };/* "%.9g" values (fp32 round-trips), no trailing commas        */
mppi_status mppi_to_csv_format(mppi_handle *h, const char *filename, int format);

/* ---- options of the Python reference's update ------------------------- */
/* clip_act (controller_base.py:500-504; the call at :453 is commented out in the reference, so off
 * by default): clamp every row of the updated sequence U' = U + Σ w·eps to [a_min[j], a_max[j]]
 * (the model's min_act()/max_act(), model_base.py:121-125) before u = U'[0] is taken.
 * n must equal a_dim; a_min = a_max = NULL switches it off. */
mppi_status mppi_set_action_limits(mppi_handle *h, const float *a_min, const float *a_max, int n);
/* filterSeq (controller_base.py:277-291): scipy.signal.savgol_filter(actionSeq, window, polyorder,
 * deriv=0, axis=0) [mode 'interp'] on the stored (shifted) sequence after every step; the smoothed
 * sequence is the next step's warm start (the reference computes it into an attribute it never
 * reads). window odd, 1 <= window <= tau, 0 <= polyorder < window; window = 0 switches it off
 * (default). The reference's literals (10, 9) have an even window, which 'interp' mode does not
 * define uniquely; they are rejected. */
mppi_status mppi_set_sequence_filter(mppi_handle *h, int window, int polyorder);

/* ---- controller state (deterministic replay; SURVEY §5 checkpoint row) ------------------ */
mppi_status mppi_get_action_sequence(mppi_handle *h, float *U, int n);        /* n = tau*a */
mppi_status mppi_set_action_sequence(mppi_handle *h, const float *U, int n);
mppi_status mppi_get_step_counter(mppi_handle *h, uint64_t *step);            /* RNG offset */
mppi_status mppi_set_step_counter(mppi_handle *h, uint64_t step);
mppi_status mppi_debug_get(mppi_handle *h, int what, float *out, size_t n);

/* ---- the reference's public graph helpers, as plain functions --------------------------- */
/* ModelBase::mBuildFreeStepGraph / mBuildActionStepGraph / mBuildModelStepGraph
 * (model_base.cpp:53-82). x is [kx,s] with kx == k or kx == 1 (broadcast initial state,
 * model_base.hpp:74-75); v is [k,a]. Any output may be NULL. out_free is [kx,s]. */
mppi_status mppi_model_step(mppi_handle *h, const float *x, int kx, const float *v, int k,
                            float *out_free, float *out_action, float *out_next);
/* AUVModel's intermediate quantities, as the reference's tests look at them one by one (scripts/test.py:264-539): for k
 * (state x[13], action u[6]) pairs -> out[k*124] = rotBtoI[9] | TBtoIquat[12] | C(nu)nu[6] | D(nu)nu[6] | g(eta)[6] | state_dot[13] |
 * D(nu)[36] | C(nu)[36]
 * (auv_model.py:353-398 body2inertial_transform, :512-545, :482-510, :450-480, :308-351). MPPI_MODEL_AUV handles only. */
mppi_status mppi_auv_pieces(mppi_handle *h, const float *x, const float *u, int k, float *out);
/* ElipseCost3D.position_error / orientation_error / velocity_error (costs/elipse_cost.py:169-246) of k states x[k*13] ->
 * out[k*3]. in_plane_frame = 1: the pose in x is ALREADY in the ellipse's plane frame (what the reference's unit tests pass to
 * the three methods); 0: the state is taken into the plane frame first, as state_cost does (:124-139).
 * MPPI_STATE_COST_ELLIPSE3D handles only. */
mppi_status mppi_ellipse3d_terms(mppi_handle *h, const float *x, int k, int in_plane_frame, float *out);
/* CostBase::mStateCost / mBuildFinalStepCostGraph (cost_base.cpp:52-61): x[k,s] -> out[k] */
mppi_status mppi_state_cost(mppi_handle *h, const float *x, int k, float *out);
/* CostBase::mActionCost (cost_base.cpp:63-68 or the Py form): u[a], eps[k,a] -> out[k] */
mppi_status mppi_action_cost(mppi_handle *h, const float *u, const float *eps, int k, float *out);
/* CostBase::mBuildStepCostGraph (cost_base.cpp:43-50): state + action cost -> out[k] */
mppi_status mppi_step_cost(mppi_handle *h, const float *x, const float *u, const float *eps, int k, float *out);
/* ControllerBase::mBuildModelGraph (controller_base.cpp:226-273): the full H-step rollout
 * cost from x[s], U[tau,a], eps[K_local,tau,a] -> cost_out[K_local]. Does not touch state. */
mppi_status mppi_rollout_cost(mppi_handle *h, const float *x, const float *U, const float *eps, float *cost_out);
/* ControllerBase::mBeta…mWeightedNoise + mBuildUpdateGraph (controller_base.cpp:166-192,
 * 215-224) on given costs: cost[K_local], eps[K_local,tau,a], U[tau,a]. Outputs (any may be
 * NULL): beta[1], exp_arg[K], exp[K], nabla[1], weights[K], weighted_noise[tau,a], U_new[tau,a]. */
mppi_status mppi_update(mppi_handle *h, const float *cost, const float *eps, const float *U,
                        float *beta, float *exp_arg, float *exp_out, float *nabla, float *weights,
                        float *weighted_noise, float *U_new);
/* ControllerBase::mGetNew / mShift(+mInit0) (controller_base.cpp:310-329), host-side slices */
mppi_status mppi_get_new(const float *U, int tau, int a, int nb, float *out);
mppi_status mppi_shift(const float *U, int tau, int a, const float *init, int nb_init, int nb, float *out);

/* ---- device-resident / asynchronous step (streams, K-sharding across GPUs) -------------- */
/* floats in one shard record: (beta_g, eta_g, V_g[tau*a]) */
int mppi_record_size(const mppi_handle *h);
/* samples this handle owns, and the global index of its first sample */
int mppi_local_samples(const mppi_handle *h);
int mppi_sample_offset(const mppi_handle *h);
/* One whole step, enqueue only: x_dev[s] -> u_dev[a]; U and the step counter advance on the
 * device. Unsharded handles only. The nominal sequence alternates between two device buffers from
 * one call to the next (the shift is a pointer offset), so a captured hipGraph must hold an EVEN
 * number of consecutive steps to be replayable (any number with a sequence filter set: the filter
 * writes back into the first buffer). */
mppi_status mppi_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream);
/* Sharded step, phase 1: rollouts + local soft-min of this shard -> record_dev[record_size]. */
mppi_status mppi_shard_partial(mppi_handle *h, const float *x_dev, float *record_dev, void *stream);
/* Sharded step, phase 2: combine n_records records (all shards, rank order — the result of an
 * all-gather) with r_g = exp(-(beta_g-beta)/λ), apply U' = U + V/η, emit u_dev[a], shift U.
 * More than 1024 records are first folded 16:1 in the handle's scratch, which holds ceil(T/16) records for the handle's own T
 * record slots (its tiles, padded): n_records must be <= 1024, or ceil(n_records/16) <= ceil(T/16). Any other count is refused
 * with MPPI_ERR_INVALID_ARG before anything is launched. */
mppi_status mppi_shard_finish(mppi_handle *h, const float *records_dev, int n_records, float *u_dev, void *stream);
/* normalize_cost on a sharded handle (controller_base.py:468-474: c' = (c - min c)/(max c - min c) over ALL K samples). Phase 1
 * splits in two around a second, 2-float exchange:
 *   mppi_shard_cost_range          rollouts of this shard; range_dev[2] = {-min, max} of ITS sample costs
 *   (the ranks reduce the pairs with ONE all-reduce(MAX): max of the -minima = -(global min), max of the maxima)
 *   mppi_shard_partial_normalized  range_dev[2] = the agreed {-min, max}: this shard's record from the costs normalised with it
 * then mppi_shard_finish as always. Same x_dev in both calls of a step; mppi_shard_partial and the direct exchange refuse such
 * a handle (MPPI_ERR_UNSUPPORTED). The result is the unsharded normalised step's up to the float rounding of the records (2e-6). */
mppi_status mppi_shard_cost_range(mppi_handle *h, const float *x_dev, float *range_dev, void *stream);
mppi_status mppi_shard_partial_normalized(mppi_handle *h, const float *x_dev, const float *range_dev, float *record_dev, void *stream);
/* ONE call per sharded step on the collective path: rollouts of this shard -> its record -> the CALLER's all-gather
 * -> combine, update, shift; enqueue only, x_dev[s] -> u_dev[a]. The library links no collective library: `coll` carries the two
 * functions with EXACTLY the signatures of ncclAllGather / ncclAllReduce (RCCL exports them under these names), so a native host
 * passes them as they are (examples/host_loop_sharded.cpp) and a Python host their addresses (mppi-tf_amd/distributed.py resolves
 * them from the librccl.so its process already holds). The library calls
 *     all_gather(own record (device, record_size floats), records (device, shard_count * record_size floats), record_size,
 *                MPPI_COLL_FLOAT32, comm, stream)          — in place: the own record IS records + shard_rank * record_size
 * and, for a normalize_cost handle only, first
 *     all_reduce(range, range, 2, MPPI_COLL_FLOAT32, MPPI_COLL_MAX, comm, stream)   — {-min, max} of the sample costs, in place
 * on the step's stream, between its own kernels. A non-zero return of either aborts the step with MPPI_ERR_EXCHANGE (nothing of
 * the update has been enqueued then; mppi_last_error carries the code). The send / receive buffers belong to the handle. With
 * shard_count == 1 and coll == NULL the collective is skipped (record -> finish on one device: the sharded sequence of kernels
 * without a communicator). Same result, bit for bit, as mppi_shard_partial -> all-gather -> mppi_shard_finish. */
enum { MPPI_COLL_FLOAT32 = 7 /* = ncclFloat32 */, MPPI_COLL_MAX = 2 /* = ncclMax */ };
typedef struct {
    int (*all_gather)(const void *sendbuff, void *recvbuff, size_t sendcount, int datatype, void *comm, void *stream);
    int (*all_reduce)(const void *sendbuff, void *recvbuff, size_t count, int datatype, int op, void *comm, void *stream); /* normalize_cost only; else may be NULL */
    void *comm; /* ncclComm_t of this rank */
} mppi_collectives;
mppi_status mppi_shard_step(mppi_handle *h, const float *x_dev, float *u_dev, const mppi_collectives *coll, void *stream);
/* Wait for the handle's own stream. */
mppi_status mppi_synchronize(mppi_handle *h);

/* ---- K-sharding, direct exchange: the records travel as peer stores inside the finish kernel --
 * A control step of the analytic model is ~25 us, of the same order as one small collective launched
 * on its own, so the exchange can also be fused into the finish kernel: every rank owns an INBOX
 * (uncached device memory) that all peers map (hipIpc across processes, peer access inside one
 * process); workgroup c of the finish kernel stores this shard's (beta_g, eta_g, V_g[c]) as 8-byte
 * {value, sequence} packets into every rank's inbox (xGMI peer stores), spins until the packets of
 * all ranks have arrived in its own, then combines them in rank order exactly as mppi_shard_finish
 * does — same bits as the all-gather path, no collective library on the step's critical path.
 * Bring-up (all ranks, same order):
 *   mppi_shard_p2p_export   allocate the inbox, get its device pointer and a 64-byte hipIpcMemHandle_t
 *   (exchange the handles out of band, e.g. over the job's bootstrap channel)
 *   mppi_shard_p2p_open     map a peer's inbox into this process (other processes' inboxes only)
 *   mppi_shard_p2p_attach   the shard_count inbox pointers in rank order (own entry = own inbox)
 *   mppi_shard_p2p_probe    one self-test round (known payload, same stores/spins); run it a few
 *                           times on every rank and agree on the outcome before trusting the path
 * then per control step mppi_shard_p2p_step on every rank (same number of calls everywhere: packets
 * carry a call sequence number). Every spin has a deadline (timeout_ms at attach); nothing hangs and nothing is
 * filled with garbage: a finish-kernel workgroup whose packets did not all arrive applies a ZERO update to its column
 * of U (the sequence still shifts, the step counter still advances) and raises a flag; launches already queued behind
 * it skip the exchange (zero updates); the next mppi_shard_p2p_step call returns MPPI_ERR_EXCHANGE and so does every
 * later one (the direct path is closed for the handle). Controls returned since the failing step are zero-update
 * controls, and U / the step counter may then differ between ranks: re-synchronise them (mppi_get/set_action_sequence,
 * mppi_get/set_step_counter from one rank) and continue with mppi_shard_partial / mppi_shard_finish, which is what
 * ShardedController.resync does. */
#define MPPI_MAX_SHARD_PEERS 16
#define MPPI_IPC_HANDLE_BYTES 64
mppi_status mppi_shard_p2p_export(mppi_handle *h, void *ipc_handle_out /* 64 B, may be NULL */, void **inbox_dev_out);
mppi_status mppi_shard_p2p_open(mppi_handle *h, const void *ipc_handle /* 64 B */, void **peer_inbox_out);
mppi_status mppi_shard_p2p_attach(mppi_handle *h, void *const *inboxes, int n, int timeout_ms);
/* ok_out = 1 if the packets of all ranks arrived with the expected payload before the deadline.
 * Synchronises the stream. */
mppi_status mppi_shard_p2p_probe(mppi_handle *h, void *stream, int *ok_out);
/* One whole sharded step, enqueue only: rollouts of this shard, exchange, update; x_dev[s] -> u_dev[a]. */
mppi_status mppi_shard_p2p_step(mppi_handle *h, const float *x_dev, float *u_dev, void *stream);
/* timed_out = 1 if any spin of any step since attach hit its deadline (complete for a step once the stream it ran
 * on has been synchronised). */
mppi_status mppi_shard_p2p_status(mppi_handle *h, int *timed_out);

/* ---- diagnostic switches (A/B timing, fault injection for the fallback tests) ----------------
 * Never needed for correct operation. The library reads NO environment variable: what a process inherits cannot
 * change kernels or inject faults; these calls are the only way. */
enum { MPPI_TUNE_FORCE_TILE_KERNEL = 0, /* 1: the LDS-tile rollout kernel instead of the producer/consumer one          */
       MPPI_TUNE_PC_PRODUCERS = 1,      /* 3 or 5 producer waves per workgroup (default: by tiles per CU)               */
       MPPI_TUNE_PC_BALANCE = 2,        /* 0: no SIMD-true role placement / progress priorities                         */
       MPPI_TUNE_PC_LDS_MIN = 3,        /* pad the rollout kernel's LDS to this many bytes (caps workgroups per CU)     */
       MPPI_TUNE_SYNC_SPIN = 4,         /* 0: mppi_next waits for the stream instead of watching the pinned u slot      */
       MPPI_TUNE_P2P_FAULT = 5,         /* 1: inbox export fails, 2: probe reports failure (exercise the RCCL fallback) */
       MPPI_TUNE_MLP_V1 = 6,            /* 1: exact-fp32 MLP rollouts on the first kernel (8 waves per workgroup) instead of k_rollout_mlp2 */
       MPPI_TUNE_MLP32_VALU = 7,        /* a Dense(32) point-mass network: 1 = k_rollout_mlp_small (vector ALU, scalar-cache weights), 2 = k_rollout_mlp32 (matrix cores, one wave
                                           per 32 rollouts) instead of k_rollout_mlp32_pc (matrix cores, network wave + cost wave per tile);
                                           NNAUVModelSpeed (Dense(16|32)): 1 = k_rollout_gen<2, HID> (vector ALU), 2 = k_rollout_nnspeed32<HID> (matrix cores, one wave per
                                           32 rollouts) instead of k_rollout_nnspeed_pc<HID> (matrix cores, network wave + pose wave per tile); NNAUVModel Dense(32):
                                           1 = k_rollout_gen<1, 32>, 2 = k_rollout_nnauv32 instead of k_rollout_nnauv_pc (network wave + cost wave per tile) */
       /* 1: roctx ranges "mppi:step" > "mppi:rollout" / "mppi:exchange" / "mppi:finish" around what every step enqueues (the reference brackets
        * its step with tf.profiler.experimental.start/stop, controller_base.py:241-248, 587-595). libroctx64.so is dlopen'ed on first use —
        * the library has no link dependency on it; the call fails with MPPI_ERR_UNSUPPORTED when it cannot be found. Shows in
        * `rocprofv3 --marker-trace`. */
       MPPI_TUNE_TRACE = 8,
       MPPI_TUNE_GEN_ONE_WAVE = 9,      /* 1: the Fossen AUVModel on k_rollout_gen<0> (one wave per 64-rollout tile) instead of k_rollout_auv_pc (pose wave + velocity wave per tile) */
       /* r05 (ABI 5), the point-mass producer/consumer path with the diagonal quadratic cost (mppi_step.hip.h): */
       MPPI_TUNE_FUSED_STEP = 10,       /* default 1: a handle of <= 128 tiles (K <= 8192) runs its Philox step as ONE launch — tiles and the column waves that
                                         * finish them in one grid, records handed over as {value, sequence} granules (seven producer waves per tile where H <= 84);
                                         * 0: rollout launch + finish launch; 2: one launch with the six-wave workgroup (five producers) at every horizon */
       MPPI_TUNE_ARMED_US = 11,         /* default 0 (off). N > 0: once two mppi_next calls have followed each other within N microseconds, a call leaves the NEXT
                                         * step's launch behind it, armed: resident on the GPU, its noise drawn, waiting up to N us for x. The next mppi_next then
                                         * only stores x into device memory (large BAR) and watches the pinned u slot — no launch, no dispatch between x and u.
                                         * While armed the launch occupies the GPU; a launch whose x does not come in time aborts by itself and changes nothing.
                                         * Controls are bit-identical to the unarmed path. MPPI_ERR_UNSUPPORTED without a large-BAR device. */
       MPPI_TUNE_ARMED_ALWAYS = 12,     /* 1: arm behind every mppi_next whatever the gap between the last two calls (tests of the deadline path) */
       MPPI_TUNE_FINISH_GENERIC = 14,   /* 1: the finish of a step on k_finish_cols (runtime record strides, every optional input decided in the kernel) instead of
                                         * k_finish_cols_cm, the column-major fast path; a batched handle: k_finish_cols_batch as it was. Same results bit for bit (A/B timing) */
       MPPI_TUNE_PRELAUNCH = 13 };      /* default 0. 1: mppi_next_device on the handle's OWN stream (stream = NULL) runs PRE-LAUNCHED: steps alternate
                                         * between two streams of the handle, the rollout of step n+1 is resident and draws its noise while step n finishes, and takes
                                         * U' of step n from the finish kernel (<= 128 tiles: from the column waves of step n's one launch) as {value, tag} granules. x_dev must be complete when the call is made and stay
                                         * unchanged until the step has run — in particular it cannot wait for u of the step before (a throughput mode, not a closed loop);
                                         * results are bit-identical to the plain path. Any other entry point drains both streams. MPPI_ERR_UNSUPPORTED for a grid of more than
                                         * one round of the chip. */
mppi_status mppi_set_tuning(mppi_handle *h, int what, int value);

/* ---- measurement (the reference only has a commented-out chrono loop, main.cpp:55-64) ------ */
/* Bracket the rollout kernel and the finish kernel of the next <= max_steps steps with HIP
 * events ON THE STREAM THEY ARE LAUNCHED ON. */
mppi_status mppi_profile_begin(mppi_handle *h, int max_steps);
/* Synchronise, stop recording, return average kernel durations in milliseconds over the
 * n_steps recorded steps (any output may be NULL). Both are the dispatches' own begin/end (what rocprofv3 reports). */
mppi_status mppi_profile_end(mppi_handle *h, float *rollout_ms_avg, float *finish_ms_avg, int *n_steps);
/* Name of the rollout kernel instance a fused step of this handle launches, as rocprofv3 prints it
 * (e.g. "mppi::k_rollout_pc<3, 3, 6, true, 0, 0>"): what a roofline figure of this handle refers to. */
mppi_status mppi_rollout_kernel_name(const mppi_handle *h, char *buf, size_t n);

/* ---- batched controllers: B independent MPPI problems stepped in the same two launches as one ------------------------------------
 * A batched handle holds n >= 1 members. mppi_create_batch_configs takes one mppi_config per member, cfgs[0..n):
 *   per member: seed, goal, lambda, gamma, upsilon, sigma and Q (diagonal or dense), with its own state and action sequence (warm-started
 *     and shifted as a lone handle's);
 *   shared, and equal in every cfgs[m] (else MPPI_ERR_INVALID_ARG naming the field and the first member that differs): k, tau, dt, mass,
 *     s_dim, a_dim, device, model_kind and the contents of auv, state_cost_kind and its parameters (quat_Q, ellipse3d), action_cost_kind,
 *     flags, q_is_full, normalize_cost, shard_rank, shard_count; also the action limits and the Philox step counter.
 * Every member must run the kernel instance member 0's lone handle runs: sigma diagonal for all members or dense for all, and Q diagonal
 * for all or dense for all (a dense Q whose off-diagonal entries are all zero counts as diagonal, as in mppi_create); a mixed batch is
 * MPPI_ERR_UNSUPPORTED naming sigma or Q. A singular sigma of member m is MPPI_ERR_SINGULAR_SIGMA naming m.
 * Member m is bit for bit the handle mppi_create(&cfgs[m]) makes, fed the same x, goal and sequence on the same step counter: sample
 * costs, beta, eta, U' and u. Members never interact. mppi_create_batch(cfg, n, seeds) is the batch of n copies of cfg with
 * seed = seeds[m].
 * Serves
 *   - the point-mass model (a_dim 1..4) with the quadratic state cost (diagonal or dense Q), every horizon the producer/consumer rollout
 *     takes (tau <= 160; <= 132 above 512 tiles);
 *   - the Fossen AUV model (MPPI_MODEL_AUV with cfg.auv; s_dim 13, a_dim 6) with the quadratic state cost (diagonal or dense Q),
 *     MPPI_STATE_COST_QUAT (StaticQuatCost) or MPPI_STATE_COST_ELLIPSE3D (ElipseCost3D), every horizon; goals are then [B, 13];
 * each with either action-cost form, diagonal or dense sigma, action limits, k <= 65536 per member.
 * Refused with MPPI_ERR_UNSUPPORTED: the MLP / NNAUV / NNAUVSpeed models, MPPI_MODEL_AUV without cfg.auv, the 2D ellipse cost (ElipseCost),
 * StaticQuatCost and ElipseCost3D without the Fossen AUV model, normalize_cost, MPPI_FLAG_FP_CONTRACT, MPPI_FLAG_MLP_BF16X3,
 * shard_count > 1; on the handle the tunings MPPI_TUNE_FUSED_STEP != 0, _ARMED_US, _PRELAUNCH and _FORCE_TILE_KERNEL (and on an AUV
 * batch _GEN_ONE_WAVE != 0 and _MLP32_VALU != 0), the sequence filter and the transition log. The per-member entry points (mppi_next,
 * mppi_next_with_noise, mppi_next_device, mppi_set_goal, mppi_get/set_action_sequence, mppi_debug_get, mppi_shard_*, the log and CSV
 * calls) refuse a batched handle with MPPI_ERR_UNSUPPORTED; mppi_destroy, mppi_synchronize, mppi_set_action_limits,
 * mppi_get/set_step_counter, mppi_profile_begin/end and mppi_rollout_kernel_name serve it as they serve a plain one. Sizes that do not
 * match, n < 1 and a member out of range are MPPI_ERR_INVALID_ARG. */
/* n members; seeds[n] their Philox keys (NULL: cfg->seed + m); every goal starts as cfg->goal, every sequence as zeros */
mppi_status mppi_create_batch(const mppi_config *cfg, int n, const uint64_t *seeds, mppi_handle **out);
/* n members, member m from cfgs[m] (its seed, goal, lambda, gamma, upsilon, sigma, Q); every sequence starts as zeros */
mppi_status mppi_create_batch_configs(const mppi_config *cfgs, int n, mppi_handle **out);
/* the member count B; 0 for a plain handle */
int mppi_batch_size(const mppi_handle *h);
/* goals[B, s] (n = B*s_dim): every member's goal (setGoal per member) */
mppi_status mppi_batch_set_goals(mppi_handle *h, const float *goals, int n);
/* one step of every member, synchronous: x[B, s] (n_x = B*s_dim) -> u_out[B, a] (n_u = B*a_dim) */
mppi_status mppi_batch_next(mppi_handle *h, const float *x, int n_x, float *u_out, int n_u);
/* the same, enqueue only: x_dev[B, s] -> u_dev[B, a] on `stream` (NULL = the handle's own; the convention of mppi_next_device) */
mppi_status mppi_batch_next_device(mppi_handle *h, const float *x_dev, float *u_dev, void *stream);
/* every member's nominal sequence U[B, tau, a] (n = B*tau*a_dim); set resets the warm start as mppi_set_action_sequence does */
mppi_status mppi_batch_get_action_sequences(mppi_handle *h, float *U, int n);
mppi_status mppi_batch_set_action_sequences(mppi_handle *h, const float *U, int n);
/* mppi_debug_get of ONE member (MPPI_DBG_*, the sizes of a lone handle) with the member's own constants: MPPI_DBG_WEIGHTS at its lambda,
 * MPPI_DBG_NOISE regenerated from its Philox key and sigma */
mppi_status mppi_batch_debug_get(mppi_handle *h, int member, int what, float *out, size_t n);

/* ---- batched learned-model controllers: one network per member --------------------------------------------------------------------
 * B controllers of the learned 13-state models (MPPI_MODEL_NN_AUV, MPPI_MODEL_NN_AUV_SPEED; s_dim 13, a_dim 6), member m with its OWN
 * network and normalisation cfgs[m].mlp, stepped in the same two launches as one. An entry point of its own, not a lifted refusal:
 * mppi_create_batch and mppi_create_batch_configs keep refusing the learned kinds word for word, because the learned batch has another
 * contract than theirs. Member m is bit for bit the lone handle mppi_create(&cfgs[m]) running the lane-per-rollout kernel
 * k_rollout_gen<MODEL, HID, DIAG> - that handle's default for NNAUVModel with Dense(16) layers, otherwise the handle tuned with
 * MPPI_TUNE_MLP32_VALU = 1 - fed the same x, goal and sequence on the same step counter: sample costs, beta, eta, U' and u. Against a lone
 * handle on its DEFAULT matrix-core pipeline (k_rollout_nnauv_pc, k_rollout_nnspeed_pc) a member agrees as those kernels agree with the
 * lane-per-rollout kernel: to rounding, inside the bars those kernels are tested to against fp64, not bit for bit. Members never
 * interact.
 *   per member: what mppi_create_batch_configs takes per member, and the network's weights and normalisation;
 *   shared (else MPPI_ERR_INVALID_ARG naming the field): what mppi_create_batch_configs shares, and the network's shape (mlp.n_layers,
 *     mlp.widths): 1-3 equal hidden layers of 16 or 32.
 * Serves every state cost a lone learned 13-state handle holds (quadratic with a diagonal or dense Q, StaticQuatCost, ElipseCost3D; the
 * quat_Q / ellipse3d parameters are shared), either action-cost form, sigma diagonal for all or dense for all, action limits, at most
 * 1024 tiles (k = 65536) per member. The handle is an ordinary batched handle: mppi_batch_next / _next_device / _set_goals /
 * _get/_set_action_sequences / _debug_get / _run_episode / _run_episode_plant, mppi_get/set_step_counter, mppi_set_action_limits,
 * mppi_synchronize, mppi_profile_begin/end, mppi_rollout_kernel_name ("mppi::k_rollout_nn_batch<1, 32, true>") and mppi_destroy serve it.
 * mppi_batch_run_episode steps member m's state with member m's own network.
 * MPPI_ERR_UNSUPPORTED, before anything is allocated: MPPI_MODEL_MLP (the learned point mass is not batched), MPPI_MODEL_POINT_MASS and
 * MPPI_MODEL_AUV (mppi_create_batch_configs serves them), normalize_cost, MPPI_FLAG_MLP_BF16X3, MPPI_FLAG_FP_CONTRACT, shard_count > 1,
 * more than 1024 tiles per member; on the handle what any batch refuses. MPPI_ERR_INVALID_ARG: NULL cfgs / out, n < 1, a member without
 * cfg.mlp, n * k too large. */
/* n members, member m from cfgs[m]: what mppi_create_batch_configs takes per member (seed, goal, lambda, gamma, upsilon, sigma, Q)
 * AND its own network cfgs[m].mlp (weights and normalisation; the descs may all be the same pointer). */
mppi_status mppi_create_batch_learned(const mppi_config *cfgs, int n, mppi_handle **out);
/* mppi_set_mlp for ONE member (member = -1: every member gets this network): same layer widths as at creation (else, and for a member
 * out of range, MPPI_ERR_INVALID_ARG and nothing changes); orders against the streams as mppi_set_mlp does; takes effect with the next
 * step. */
mppi_status mppi_batch_set_mlp(mppi_handle *h, int member, const mppi_mlp_desc *mlp);

/* ---- batched learned point-mass controllers: one MLP per member ---------------------------------------------------------------------
 * B controllers of MPPI_MODEL_MLP (s_dim = 2 a_dim), member m with its OWN network and normalisation cfgs[m].mlp, stepped in the same two
 * launches as one. An entry point of its own: mppi_create_batch, mppi_create_batch_configs and mppi_create_batch_learned keep refusing
 * MPPI_MODEL_MLP word for word. Member m is bit for bit the lone handle mppi_create(&cfgs[m]) fed the same x, goal and sequence on the
 * same step counter - sample costs, beta, eta, U' and u - where that handle runs
 *   the [3a, 256, 256, 2a] network, a_dim 1..3:  k_rollout_mlp2<A, DIAG, SRC_PHILOX>, its DEFAULT matrix-core kernel (the batch runs the same
 *                                                kernel body with a member axis, k_rollout_mlp2_batch<A, DIAG>);
 *   Dense(16) x 1..3, a_dim 1..4:                k_rollout_mlp_small<A, 16>, its default (k_rollout_mlp_small_batch<A, 16>);
 *   Dense(32) x 1..3, a_dim 1..4:                k_rollout_mlp_small<A, 32>, the handle tuned MPPI_TUNE_MLP32_VALU = 1; against that handle's
 *                                                default k_rollout_mlp32_pc a member agrees to rounding, inside the bars both kernels are
 *                                                tested to against fp64, not bit for bit.
 * Members never interact.
 *   per member: seed, goal, lambda, gamma, upsilon, sigma, the diagonal Q, and the network's weights and normalisation;
 *   shared (else MPPI_ERR_INVALID_ARG naming the field, e.g. "cfgs[1].mlp.widths"): what mppi_create_batch_configs shares, and the
 *     network's shape (mlp.n_layers, mlp.widths).
 * The handle is an ordinary batched handle: mppi_batch_next / _next_device / _set_goals / _get/_set_action_sequences / _debug_get /
 * _set_mlp / _run_episode / _run_episode_plant, mppi_get/set_step_counter, mppi_set_action_limits, mppi_synchronize,
 * mppi_profile_begin/end, mppi_rollout_kernel_name ("mppi::k_rollout_mlp2_batch<3, true>") and mppi_destroy serve it.
 * mppi_batch_run_episode steps member m's state with member m's own network; in mppi_batch_run_episode_plant a learned plant stays shared.
 * MPPI_ERR_UNSUPPORTED, before anything is allocated, the message naming the cause: another model kind (POINT_MASS, AUV:
 * mppi_create_batch_configs serves them; NN_AUV, NN_AUV_SPEED: mppi_create_batch_learned), the {256, 256} network at a_dim = 4 (the lone
 * handle runs k_rollout_mlp there, which this batch does not carry), normalize_cost, MPPI_FLAG_MLP_BF16X3, MPPI_FLAG_FP_CONTRACT,
 * shard_count > 1, a dense Q (q_is_full), a state cost other than the quadratic one, more than 1024 tiles per member; on the handle what
 * any batch refuses (the tunings of the lone step, MPPI_TUNE_MLP32_VALU, MPPI_TUNE_MLP_V1, the sequence filter, the transition log,
 * mppi_set_mlp). MPPI_ERR_INVALID_ARG: NULL cfgs / out, n < 1, a member without cfg.mlp, a member whose shared field or network shape
 * differs from member 0's, sigma diagonal for some members and dense for others, n * k too large. */
mppi_status mppi_create_batch_mlp(const mppi_config *cfgs, int n, mppi_handle **out);

/* ---- closed-loop episodes: n_steps control steps on the device, the handle's own model as the plant ---------------------------------
 * For t = 0 .. n_steps-1, per member:
 *   1. goals given: goal <- goals[t] (the effect of mppi_set_goal / mppi_batch_set_goals before the step);
 *   2. C[t] = the state cost of x_t under that goal (mppi_state_cost's value);
 *   3. U[t] = the control of one ordinary step from x_t: what mppi_next_device on the handle's own stream runs (one launch, two, or the
 *      normalize_cost passes; action limits and the sequence filter apply), never the pre-launched or an armed step; a batch: its batched step;
 *   4. x_{t+1} = model(x_t, U[t]), bit for bit mppi_model_step's out_next;
 *   5. disturbance given: x_{t+1} = x_{t+1} + w_t, a raw fp32 add per component (keep a 13-state model's quaternion entries at zero);
 *   6. X[0] = x0, X[t+1] = x_{t+1}.
 * All steps are enqueued on the handle's own stream without a host wait between them; the call returns after one synchronisation. Behind
 * every control step ONE more launch closes the loop (a learned model: two). Afterwards the handle is where the host loop "set goal, next,
 * model_step" repeated n_steps times leaves it: the sequence warm-started and shifted n_steps times, the step counter advanced by n_steps,
 * the goal equal to the last row of goals; a second call continues where the first stopped. The transition log is not written: X, U and
 * C are the episode's log. Host pointers; goals, disturbance and each output may be NULL.
 * MPPI_ERR_INVALID_ARG: n_steps < 1, a wrong n_x, x0 NULL, a sharded handle (as mppi_next_device), mppi_batch_run_episode on a lone
 * handle. MPPI_ERR_UNSUPPORTED: mppi_run_episode on a batched handle, a handle that runs no rollouts. Nothing is enqueued before a refusal. */
/* lone handle: x0[s] (n_x = s_dim), goals / disturbance [n_steps, s] -> X[n_steps+1, s], U[n_steps, a], C[n_steps] */
mppi_status mppi_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                             float *X_out, float *U_out, float *C_out);
/* batched handle, a member axis after the step axis: x0[B, s] (n_x = B*s_dim), goals / disturbance [n_steps, B, s] ->
 * X[n_steps+1, B, s], U[n_steps, B, a], C[n_steps, B] */
mppi_status mppi_batch_run_episode(mppi_handle *h, const float *x0, int n_x, int n_steps, const float *goals, const float *disturbance,
                                   float *X_out, float *U_out, float *C_out);

/* ---- ... against a separate plant: the model of ANOTHER handle steps the state ---------------------------------------------------------
 * mppi_run_episode / mppi_batch_run_episode in every respect (the goal per step, C[t] under the controller's cost and goal, the ordinary
 * control step, the raw fp32 add of the disturbance, where the handle ends) but step 4:
 *   4. x_{t+1} = model_of(plants[m])(x_t, U[t]) for member m (plants[0] when n_plants is 1), bit for bit what mppi_model_step on that
 *      plant handle returns as out_next.
 * A plant is an ordinary lone, unsharded handle on the controller's device with the controller's s_dim and a_dim. Only its model is used:
 * mass and dt of the point mass, the mppi_auv_desc of the Fossen model, the network of a learned model. Its cost, goal, action sequence,
 * step counter and log are neither read nor written; it may be a handle that runs no rollouts (k = 1, tau = 1), and it may be h itself.
 * n_plants is 1 (every member shares the plant; the only value for a lone controller) or B (member m steps with plants[m]).
 * Served: every controller mppi_run_episode / mppi_batch_run_episode serves, with any plant model of its dimensions — a learned
 * controller on the Fossen plant, a Fossen controller on a learned plant, a point mass on a point mass of another mass or dt, ... Plants
 * per member (n_plants = B > 1) are served for the analytic models, the point mass and the Fossen model. A learned plant is shared
 * (n_plants = 1): its model-step kernel takes one launch over the B rows.
 * Everything is enqueued on the CONTROLLER's stream, with one synchronisation at the end; the launches per step are those of the plain
 * episode. Each plant's own stream is synchronised once at entry, so that an mppi_set_mlp in flight on a plant is complete before its
 * weights are read. Plants are only read, and nothing outlives the call.
 * MPPI_ERR_INVALID_ARG: plants NULL or an entry NULL, n_plants not 1 or B, a batched or a sharded plant, a plant whose s_dim, a_dim or
 * device differs from the controller's. MPPI_ERR_UNSUPPORTED: learned plants per member, a plant whose model does not step the
 * controller's state layout. Every refusal of mppi_run_episode / mppi_batch_run_episode applies, the lone entry point on a batched handle
 * and the reverse included. Nothing is enqueued before a refusal. */
mppi_status mppi_run_episode_plant(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                   const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out);
mppi_status mppi_batch_run_episode_plant(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                         const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out);

/* ---- step statistics: what the observer logs per control step (observer_base.py:101-187), computed on the device -------------------------
 * The MPPI_DBG_* items are the raw arrays of the last step; these are the per-step scalars and histograms a user tunes lambda by, read from
 * the same buffers (the sample costs, beta, eta, the cost buffer and temperature MPPI_DBG_WEIGHTS weighs) by ONE launch, one workgroup per
 * member, fp64 sums in a fixed order (no float atomics): the same inputs give the same bits. Per sample k, exactly MPPI_DBG_WEIGHTS'
 * quantities: arg_k = t (c'_k - beta) in fp32 (t = -1/lambda, or the step's temperature under normalize_cost; c' the costs the weights were
 * made from), e_k = expf(arg_k). A sample whose raw cost (MPPI_DBG_COSTS) is not finite is counted in N_NONFINITE and left out of every
 * sum, maximum and histogram. stats[MPPI_N_STEP_STATS] per member: */
#define MPPI_N_STEP_STATS 9
#define MPPI_STEP_STAT_BINS 32
enum { MPPI_STAT_BETA = 0,        /* MPPI_DBG_BETA, the bits unchanged                                                              */
       MPPI_STAT_ETA = 1,         /* MPPI_DBG_ETA, the bits unchanged (the observer's nabla; Nabla_percent = ETA / K)               */
       MPPI_STAT_ESS = 2,         /* effective sample size (sum e)^2 / sum e^2, from the launch's own sums: 1 .. K                  */
       MPPI_STAT_ENTROPY = 3,     /* -sum w ln w of the weights w = e / sum e, as ln S1 - (sum e arg) / S1: 0 .. ln K               */
       MPPI_STAT_COST_MEAN = 4,   /* mean of the finite raw costs                                                                   */
       MPPI_STAT_COST_STD = 5,    /* their population standard deviation (second pass, about the mean)                              */
       MPPI_STAT_COST_MAX = 6,    /* the largest finite raw cost                                                                    */
       MPPI_STAT_BEST_INDEX = 7,  /* the lowest k whose raw cost is the smallest finite one (the observer's best_id); exact as a float */
       MPPI_STAT_N_NONFINITE = 8  /* how many raw costs are not finite                                                              */ };
/* hist_cost[32] (the observer's All_cost): linear bins over [cmin, COST_MAX] of the finite raw costs, bin = min(31, (int)((c - cmin) *
 * (32.0f / (COST_MAX - cmin)))) in fp32, every sample in bin 0 when COST_MAX = cmin. hist_weight[32] (exponenetial_argument / Weights):
 * octaves below the best sample, bin = min(31, (int)(-arg * 1.442695f)): bin j holds the samples whose weight lies in (2^-(j+1), 2^-j] of
 * the best one's. Both sum to K_local - N_NONFINITE. Without a finite cost the five statistics of indices 2..6 are NaN and BEST_INDEX -1.
 * Statistics of the LAST step of the handle (mppi_next*, mppi_batch_next*, an episode's last step); synchronous; host pointers, any of
 * which may be NULL. They only observe: nothing a step reads is written. A pre-launched pipeline is drained and an armed launch retired
 * first, as by any entry point (neither leaves a cost or beta of a step that did not complete).
 * MPPI_ERR_INVALID_ARG: no step has run yet (or mppi_update has overwritten beta and eta since), mppi_batch_step_stats on a lone handle.
 * MPPI_ERR_UNSUPPORTED: mppi_step_stats on a batched handle, a sharded handle (the costs of one rank are not the step's), 2^24 or more
 * samples per member (BEST_INDEX would not be exact). Nothing is enqueued before a refusal. */
mppi_status mppi_step_stats(mppi_handle *h, float *stats /* [9] */, uint32_t *hist_cost /* [32] */, uint32_t *hist_weight /* [32] */);
mppi_status mppi_batch_step_stats(mppi_handle *h, float *stats /* [B, 9] */, uint32_t *hist_cost /* [B, 32] */, uint32_t *hist_weight /* [B, 32] */);
/* mppi_run_episode / mppi_run_episode_plant (plants == NULL and n_plants == 0: the handle's own model) with the statistics of EVERY step
 * logged: one more launch per step, enqueued right behind the control step; the rows travel in the episode's staging and are copied out
 * with X, U and C — no host wait inside. X, U, C and where the handle ends are bit for bit the plain episode's. The batched entry has a
 * member axis after the step axis. Every refusal of the plain episodes and of mppi_step_stats (but "no step has run yet") applies. */
mppi_status mppi_run_episode_stats(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                   const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out,
                                   float *S_out /* [n_steps, 9] */, uint32_t *Hc_out /* [n_steps, 32] */, uint32_t *Hw_out /* [n_steps, 32] */);
mppi_status mppi_batch_run_episode_stats(mppi_handle *h, mppi_handle *const *plants, int n_plants, const float *x0, int n_x, int n_steps,
                                         const float *goals, const float *disturbance, float *X_out, float *U_out, float *C_out,
                                         float *S_out /* [n_steps, B, 9] */, uint32_t *Hc_out /* [n_steps, B, 32] */,
                                         uint32_t *Hw_out /* [n_steps, B, 32] */);

/* ---- open-loop rollouts: the handle's model rolled along n GIVEN action sequences, every state and its cost written out ------------------
 * "Where does this model go if I apply these actions?" in one call with no host wait inside: the nominal plan, the plan of a chosen sample
 * (V = U + eps[k]), or the H-step open-loop error of a learned model along recorded actions. The step axis comes first and the trajectory
 * axis after it, as in the episodes' X[n_steps+1, B, s]:
 *   x0[kx, s] with kx in {1, n} (one start shared by all trajectories, or one each), V[T, n, a] -> X[T+1, n, s], C[T, n].
 * For trajectory i:
 *   X[0, i] = x0[kx == 1 ? 0 : i];
 *   X[t+1, i] = model(X[t, i], V[t, i]) for t = 0 .. T-1, bit for bit what mppi_model_step returns as out_next;
 *   C[t, i] = the state cost of X[t+1, i] under the handle's current goal, bit for bit mppi_state_cost's value: the state the step
 *     PRODUCED, which is the post-step state a rollout of the control step charges (the terminal cost the rollouts add once more is
 *     C[T-1, i] again; no action cost is computed here).
 * T is any value >= 1, not tied to the handle's tau. The analytic models (the point mass, the Fossen model) run ONE launch: a lane per
 * trajectory, the step loop inside the kernel. A learned model (MPPI_MODEL_MLP, NN_AUV, NN_AUV_SPEED) runs T launches of the exactly-ordered
 * reference kernel behind mppi_model_step and one cost launch: its trajectory here is that REFERENCE-ORDERED evaluation, as with
 * mppi_model_step — the matrix-core rollout kernels of a control step round differently.
 * Served: every lone handle mppi_model_step serves, handles that run no rollouts (k = 1, tau = 1) included — the point mass and
 * MPPI_MODEL_MLP with a_dim 1..4 (s_dim = 2 a_dim), the three 13-state models — with every state cost the handle can hold.
 * Only the model and the cost with its goal are read: the action sequence, the step counter, the goal, the handle's x, its cost and record
 * buffers and the transition log are neither read nor written, and an mppi_next after the call returns what it would have returned
 * without it.
 * MPPI_ERR_UNSUPPORTED: a batched handle (its members share one model: roll it on a lone handle), a point-mass or MLP handle with
 * a_dim > 4. MPPI_ERR_INVALID_ARG: n < 1, T < 1 (or n * T > 2^30), kx not 1 or n, x0 or V NULL, no output. Nothing is enqueued before a
 * refusal. */
/* host pointers; one synchronisation at the end. Either output may be NULL, not both. */
mppi_status mppi_model_rollout(mppi_handle *h, const float *x0, int kx, const float *V, int n, int T,
                               float *X_out, float *C_out);
/* device pointers, enqueue only on `stream` (NULL = the handle's own; the convention of mppi_next_device). X_dev is required (a learned
 * model steps from row to row of it); C_dev may be NULL: no cost arithmetic. A learned model's per-row scratch belongs to the handle:
 * a call on another stream than the previous call's first waits for that stream, which must still exist. */
mppi_status mppi_model_rollout_device(mppi_handle *h, const float *x0_dev, int kx, const float *V_dev, int n, int T,
                                      float *X_dev, float *C_dev, void *stream);

/* ---- the learner of the learned model_base (replaces LearnerBase.train / _train_step, learners/learner_base.py:324-358,
 * 469-496; train_all :146-153) --------------------------------------------------------------------------------------------
 * Full-batch Adam on the mean squared error of the network's prediction against the (normalised) targets, for the
 * reference's Dense networks (nn_model.py:54-60; widths <= 32, 1-4 layers, relu on the hidden layers) and for exactly the network an
 * MPPI_MODEL_MLP controller rolls out: n_layers = 3, widths = [in, 256, 256, out] with in, out <= 32 (the "wide" learner: every product
 * on the exact-fp32 matrix-core instruction). Any other shape is MPPI_ERR_UNSUPPORTED. The data preparation
 * (prepare_training_data, normalisation statistics, augmentation) is host bookkeeping in the caller; what runs on the
 * device is forward, loss, backward (the weight-gradient GEMMs over the batch on the matrix cores, exact fp32) and the Adam
 * update — a train loop of many steps needs no host round trip. Its weights are what mppi_config.mlp of an
 * MPPI_MODEL_NN_AUV / MPPI_MODEL_MLP controller takes. Deterministic (no float atomics). Not thread-safe per learner. */
typedef struct mppi_learner mppi_learner;
/* widths[n_layers + 1] = inputs, hidden widths..., outputs; W[l] is [widths[l] x widths[l+1]] row-major (Keras kernel), b[l] [widths[l+1]] */
mppi_status mppi_learner_create(int n_layers, const int32_t *widths, const float *const *W, const float *const *b, int device,
                                mppi_learner **out);
void mppi_learner_destroy(mppi_learner *l);
const char *mppi_learner_last_error(const mppi_learner *l);
/* the training set: X [n, inputs], Y [n, outputs] (copied to the device) */
mppi_status mppi_learner_set_data(mppi_learner *l, const float *X, const float *Y, int n);
/* `steps` Adam steps (tf.optimizers.Adam's update: m, v, lr*sqrt(1-b2^t)/(1-b1^t), eps outside the root; Keras defaults
 * beta1 0.9, beta2 0.999, eps 1e-7). loss_first / loss_last (may be NULL): the loss of the first / last step's forward pass. */
mppi_status mppi_learner_train(mppi_learner *l, int steps, float lr, float beta1, float beta2, float eps, float *loss_first, float *loss_last);
/* loss of the CURRENT weights on the training set, no update; grads_out (NULL or [n_layers*33*32]: per layer rows 0..31 = dLoss/dW
 * padded to 32 x 32, row 32 = dLoss/db; widths <= 32 only: on a [in, 256, 256, out] learner a non-NULL grads_out is MPPI_ERR_UNSUPPORTED,
 * use mppi_learner_gradients) ; pred_out (NULL or [n, outputs]) */
mppi_status mppi_learner_evaluate(mppi_learner *l, float *loss_out, float *grads_out, float *pred_out);
/* loss and gradients of the CURRENT weights on the training set, no update; dW[l] is [widths[l] x widths[l+1]] row-major, db[l] [widths[l+1]]
 * (the layout of mppi_learner_get_weights). Any of loss_out, dW, db may be NULL. Every learner. */
mppi_status mppi_learner_gradients(mppi_learner *l, float *loss_out, float *const *dW, float *const *db);
mppi_status mppi_learner_get_weights(mppi_learner *l, float *const *W, float *const *b);
mppi_status mppi_learner_set_weights(mppi_learner *l, const float *const *W, const float *const *b);
/* forget the Adam moments and the step count (a new tf.optimizers.Adam, learner_base.py:149) */
mppi_status mppi_learner_reset_optimizer(mppi_learner *l);
mppi_status mppi_learner_get_step(mppi_learner *l, int *step);
/* Persistence (replaces NNModel.save_params / load_params, models/nn_model.py:137-142 — a Keras SavedModel there — and
 * LearnerBase.save_params, learners/learner_base.py:66-68; the reference does not keep its optimizer state, this does, so that a resumed
 * run continues bit for bit). ONE flat little-endian file:
 *     char    magic[8] = "MPPILRN1"
 *     int32   n_layers, widths[5] (n_layers + 1 used, rest 0), adam_step, has_norm
 *     per layer l (in = widths[l], out = widths[l+1]), fp32, compact:  W[in][out] b[out]  mW[in][out] mb[out]  vW[in][out] vb[out]
 *     if has_norm, fp64:  xmean[widths[0]] xstd[widths[0]] ymean[widths[n_layers]] ystd[widths[n_layers]]
 * (the normalisation belongs to the model, not to the learner: the caller passes it in and gets it back; all four NULL = none).
 * The widths are those mppi_learner_create takes (<= 32, or [in, 256, 256, out]); a file of anything else is MPPI_ERR_IO.
 * mppi_learner_save writes beside the target and renames over it. mppi_learner_load: the learner's layer widths must match (mppi_learner_peek
 * reads them from a file, to create the learner with); weights, both Adam moments and the step count are replaced; *has_norm says whether the
 * file held a normalisation (the four outputs are written only then; they may be NULL). */
mppi_status mppi_learner_save(mppi_learner *l, const char *filename, const double *xmean, const double *xstd, const double *ymean, const double *ystd);
mppi_status mppi_learner_load(mppi_learner *l, const char *filename, double *xmean, double *xstd, double *ymean, double *ystd, int *has_norm);
mppi_status mppi_learner_peek(const char *filename, int *n_layers, int32_t *widths /* [5] */);

/* ---- batched learners: B narrow learners in the launches of one (replaces LearnerBase.k_fold_validation / grid_search,
 * learners/learner_base.py:83-216: k copies of the network, one per fold, each with its own Adam, over a grid of rates).
 * n_members 1..1024 (else MPPI_ERR_INVALID_ARG); the network is the narrow learner's (n_layers 1..4, widths 1..32, layout of
 * mppi_learner_create); [in, 256, 256, out] and whatever mppi_learner_create refuses is MPPI_ERR_UNSUPPORTED, checked before the device
 * is touched. Every member starts from the same W, b.
 * Data: ONE pool X [n, in], Y [n, out] for all members (mppi_learner_batch_set_data; it resets every split). Member m trains on the
 * rows train_idx[0..n_train) in that order and reports its held-out loss over test_idx[0..n_test) (mppi_learner_batch_set_split;
 * indices may repeat, n_train >= 1, n_test >= 0; an index outside [0, n) is MPPI_ERR_INVALID_ARG and nothing changes). Before any
 * set_split a member trains on rows 0..n-1 and has no test rows.
 * One step is the lone learner's step for every member, each with its own lr, beta1, beta2, eps ([B] arrays; NULL = 0.9 / 0.999 /
 * 1e-7); one step counter serves the batch. loss_train[t * B + m] is the loss of step t's forward pass before its update
 * (mppi_learner_train's loss_first of a one-step call); loss_test[t * B + m] is the loss of the weights AFTER step t's update on the
 * member's test rows (kfold_step: _train_step, then evaluate), NaN for a member without test rows. mppi_learner_batch_train enqueues
 * every step on the object's own stream and synchronises once; mppi_learner_batch_evaluate returns both losses of the current weights
 * without an update.
 * The contract: member m is bit-identical — weights, loss_train, loss_test — to a lone mppi_learner created with the same weights,
 * given mppi_learner_set_data(X[train_idx_m], Y[train_idx_m]) and trained with member m's rates (its loss_test: mppi_learner_evaluate of
 * a lone learner holding the member's weights on X[test_idx_m], Y[test_idx_m]). Members never interact. Deterministic (no float
 * atomics). The activations are [B][layers][max n_train][32] floats: a large B x n can be MPPI_ERR_ALLOC. Not thread-safe per object.
 * Errors as the learner's: mppi_learner_batch_last_error(NULL) after a failed create. */
typedef struct mppi_learner_batch mppi_learner_batch;
mppi_status mppi_learner_batch_create(int n_members, int n_layers, const int32_t *widths, const float *const *W, const float *const *b,
                                      int device, mppi_learner_batch **out);
void mppi_learner_batch_destroy(mppi_learner_batch *lb);
const char *mppi_learner_batch_last_error(const mppi_learner_batch *lb);
int mppi_learner_batch_size(const mppi_learner_batch *lb);
mppi_status mppi_learner_batch_set_data(mppi_learner_batch *lb, const float *X, const float *Y, int n); /* the shared pool */
mppi_status mppi_learner_batch_set_split(mppi_learner_batch *lb, int member, const int32_t *train_idx, int n_train,
                                         const int32_t *test_idx, int n_test);
mppi_status mppi_learner_batch_set_weights(mppi_learner_batch *lb, int member /* -1: every member */, const float *const *W, const float *const *b);
mppi_status mppi_learner_batch_get_weights(mppi_learner_batch *lb, int member, float *const *W, float *const *b);
mppi_status mppi_learner_batch_reset_optimizer(mppi_learner_batch *lb);
mppi_status mppi_learner_batch_get_step(mppi_learner_batch *lb, int *step);
mppi_status mppi_learner_batch_train(mppi_learner_batch *lb, int steps, const float *lr /* [B] */, const float *beta1, const float *beta2,
                                     const float *eps /* each [B] or NULL = 0.9 / 0.999 / 1e-7 */,
                                     float *loss_train /* [steps, B] or NULL */, float *loss_test /* [steps, B] or NULL */);
mppi_status mppi_learner_batch_evaluate(mppi_learner_batch *lb, float *loss_train /* [B] */, float *loss_test /* [B] */);

/* ---- trajectory validation of the members (LearnerBase.validate_fold; learner_base.py:181-188, 211-216 roll each fold's model along
 * held-out action sequences every tenth epoch): every member's network, as the learned model `model` describes it, rolled open-loop
 * along n action sequences of T steps in ONE launch on the batch's stream, one synchronisation. Host pointers; layouts as
 * mppi_model_rollout: x0 [kx, s_dim] with kx = 1 (shared) or n, V [T, n, a_dim], G [T+1, n, s_dim] the ground truth.
 *   X_out[m, 0, i] = x0, X_out[m, t+1, i] = model_m(X_out[m, t, i], V[t, i]): bit for bit what mppi_model_rollout returns on a lone
 *     handle of that model kind holding member m's weights and this normalisation (the reference-ordered evaluation of mppi_model_step).
 *   sse_out[m, j] = sum over t = 0..T and i of (X[m, t, i, j] - G[t, i, j])^2: fp32 per trajectory (t ascending) and per 64 trajectories
 *     (a fixed butterfly), then the blocks of 64 in order in fp64. A member whose trajectories overflow reports a non-finite sse of its
 *     own; the other members are unaffected. Deterministic.
 * The batch's weights, Adam moments, data, splits and step counter are neither written nor, but for the weights, read.
 * Refused before the device is touched, the batch stays usable: MPPI_ERR_INVALID_ARG for model, x0 or V NULL, both outputs NULL, sse_out
 * without G, n < 1, T < 1, n * T > 2^30, kx not 1 or n, an xstd entry equal to 0; MPPI_ERR_UNSUPPORTED for a model_kind outside the three
 * and for a network whose first / last width is not the kind's (MPPI_MODEL_MLP: s_dim + a_dim -> s_dim with s_dim = 2 a_dim, a_dim <= 4;
 * MPPI_MODEL_NN_AUV: 16 -> 13 and MPPI_MODEL_NN_AUV_SPEED: 15 -> 6, both s_dim = 13, a_dim = 6). */
typedef struct {
    int32_t model_kind;          /* MPPI_MODEL_MLP | MPPI_MODEL_NN_AUV | MPPI_MODEL_NN_AUV_SPEED */
    int32_t s_dim, a_dim;
    float   dt;                  /* NN_AUV_SPEED only */
    const float *xmean, *xstd;   /* [net inputs]; NULL = 0 / 1 */
    const float *ymean, *ystd;   /* [net outputs]; NULL = 0 / 1 */
} mppi_learner_model;
mppi_status mppi_learner_batch_rollout(mppi_learner_batch *lb, const mppi_learner_model *model,
                                       const float *x0 /* [kx, s], kx in {1, n} */, int kx, const float *V /* [T, n, a] */,
                                       const float *G /* [T+1, n, s] or NULL */, int n, int T,
                                       double *sse_out /* [B, s] or NULL; needs G */, float *X_out /* [B, T+1, n, s] or NULL */);

/* ---- batched WIDE learners: B learners of the [in, 256, 256, out] network (the one mppi_learner_create accepts beside the narrow shapes,
 * the network of an MPPI_MODEL_MLP controller) in the launches of one — mppi_learner_batch_* restated for that network, as an object of its
 * own (mppi_learner_batch_create goes on refusing the shape). The entry points are the namesakes' with the object type exchanged.
 * n_members 1..1024 (else MPPI_ERR_INVALID_ARG); n_layers = 3 and widths[4] exactly [1..32, 256, 256, 1..32], anything else is
 * MPPI_ERR_UNSUPPORTED; both checked before the device is touched. Every member starts from the same W, b.
 * Data: ONE pool X [n, in], Y [n, out] for all members (set_data; it resets every split). Member m trains on the rows
 * train_idx[0..n_train) in that order and reports its held-out loss over test_idx[0..n_test) (set_split; indices may repeat, n_train >= 1,
 * n_test >= 0; an index outside [0, n) is MPPI_ERR_INVALID_ARG and nothing changes). Before any set_split a member trains on rows 0..n-1
 * and has no test rows.
 * lr, beta1, beta2, eps per member ([B] arrays; NULL = 0.9 / 0.999 / 1e-7); one step counter serves the batch. loss_train[t * B + m] is
 * the loss of step t's forward pass before its update; loss_test[t * B + m] is the loss of the weights AFTER step t's update on the
 * member's test rows, NaN for a member without test rows. train enqueues every step on the object's own stream (nine launches per step
 * for any B, twelve with test losses) and synchronises once; evaluate returns both losses of the current weights without an update.
 * The contract: member m is bit-identical — weights, loss_train, loss_test — to a lone [in, 256, 256, out] mppi_learner created with the
 * same weights, given mppi_learner_set_data(X[train_idx_m], Y[train_idx_m]) and trained with member m's rates from the same step count
 * (its loss_test: mppi_learner_evaluate of a lone learner holding the member's weights on X[test_idx_m], Y[test_idx_m]). Members never
 * interact. Deterministic (no float atomics). A member costs 1.0 MB of weights and moments, 0.33 MB of partial tiles per 512 training rows
 * of the largest split and 4.4 KB of rows, activations and deltas per row of the largest split: a batch too large for the device is MPPI_ERR_ALLOC and the object stays destroyable (and usable
 * after smaller splits). Not thread-safe per object. Errors as the learner's: mppi_learner_wide_batch_last_error(NULL) after a failed create.
 * Trajectory validation of a wide batch is mppi_learner_wide_batch_validate below: an entry point of its own — mppi_learner_batch_rollout
 * stays narrow-only and has no wide namesake. */
typedef struct mppi_learner_wide_batch mppi_learner_wide_batch;
mppi_status mppi_learner_wide_batch_create(int n_members, int n_layers /* 3 */, const int32_t *widths /* [4] */, const float *const *W,
                                           const float *const *b, int device, mppi_learner_wide_batch **out);
void mppi_learner_wide_batch_destroy(mppi_learner_wide_batch *wb);
const char *mppi_learner_wide_batch_last_error(const mppi_learner_wide_batch *wb);
int mppi_learner_wide_batch_size(const mppi_learner_wide_batch *wb);
mppi_status mppi_learner_wide_batch_set_data(mppi_learner_wide_batch *wb, const float *X, const float *Y, int n); /* the shared pool */
mppi_status mppi_learner_wide_batch_set_split(mppi_learner_wide_batch *wb, int member, const int32_t *train_idx, int n_train,
                                              const int32_t *test_idx, int n_test);
mppi_status mppi_learner_wide_batch_set_weights(mppi_learner_wide_batch *wb, int member /* -1: every member */, const float *const *W,
                                                const float *const *b);
mppi_status mppi_learner_wide_batch_get_weights(mppi_learner_wide_batch *wb, int member, float *const *W, float *const *b);
mppi_status mppi_learner_wide_batch_reset_optimizer(mppi_learner_wide_batch *wb);
mppi_status mppi_learner_wide_batch_get_step(mppi_learner_wide_batch *wb, int *step);
mppi_status mppi_learner_wide_batch_train(mppi_learner_wide_batch *wb, int steps, const float *lr /* [B] */, const float *beta1,
                                          const float *beta2, const float *eps /* each [B] or NULL = 0.9 / 0.999 / 1e-7 */,
                                          float *loss_train /* [steps, B] or NULL */, float *loss_test /* [steps, B] or NULL */);
mppi_status mppi_learner_wide_batch_evaluate(mppi_learner_wide_batch *wb, float *loss_train /* [B] */, float *loss_test /* [B] */);
/* ---- trajectory validation of the wide members: mppi_learner_batch_rollout's arguments and meaning for the [3a, 256, 256, 2a] network.
 * Every member's network, as the MPPI_MODEL_MLP `model` describes it, rolled open-loop along n action sequences of T steps in ONE launch
 * (k_wb_rollout: vector-ALU fp32 in the plain order, not the learner's matrix-core tiles) on the batch's stream, behind any training in
 * flight; one synchronisation at the end. Host pointers.
 *   X_out[m, 0, i] = x0, X_out[m, t+1, i] = model_m(X_out[m, t, i], V[t, i]): bit for bit what mppi_model_rollout returns on a lone
 *     MPPI_MODEL_MLP handle holding member m's weights and this normalisation.
 *   sse_out[m, j] = sum over t = 0..T and i of (X[m, t, i, j] - G[t, i, j])^2: fp32 per trajectory (t ascending) and per 16 trajectories
 *     (a fixed pairwise tree), then the blocks of 16 in order in fp64. A member whose trajectories overflow reports a non-finite sse of its
 *     own; the other members are unaffected. Deterministic.
 * Only the weights are read: Adam moments, step counter, data and splits are untouched, and the next train returns the bits it would have
 * returned. The call's device buffers are its own, grown on demand and freed by mppi_learner_wide_batch_destroy.
 * Refused before the device is touched, the batch stays usable: MPPI_ERR_INVALID_ARG for model, x0 or V NULL, both outputs NULL, sse_out
 * without G, n < 1, T < 1, n * T > 2^30, kx not 1 or n, an xstd entry equal to 0; MPPI_ERR_UNSUPPORTED for a model_kind other than
 * MPPI_MODEL_MLP, for s_dim != 2 a_dim or a_dim outside 1..4, and for a batch whose widths are not [3 a_dim, 256, 256, 2 a_dim]. */
mppi_status mppi_learner_wide_batch_validate(mppi_learner_wide_batch *wb, const mppi_learner_model *model,
                                             const float *x0 /* [kx, s], kx in {1, n} */, int kx, const float *V /* [T, n, a] */,
                                             const float *G /* [T+1, n, s] or NULL */, int n, int T,
                                             double *sse_out /* [B, s] or NULL; needs G */, float *X_out /* [B, T+1, n, s] or NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MPPI_C_H_ */
