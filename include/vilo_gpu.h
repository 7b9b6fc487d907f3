/* vilo_gpu.h — C ABI of the MI355X-native sliding-window VILO solver.
 *
 * Drop-in boundary for the hot path of ShuoYangRobotics/Cerberus:
 *     void Estimator::optimization()          src/estimator/estimator.cpp:1054-1458
 * i.e. per-frame nonlinear least squares over the 11-frame window (IMU-leg contact-preintegration
 * factors, stereo reprojection factors, marginalisation prior; Ceres DENSE_SCHUR + DOGLEG) followed by
 * Schur-complement marginalisation. All entry points take plain pointers and sizes; there are no
 * torch / Eigen / Ceres types in any signature. Everything is FP64, like the reference.
 *
 * Each entry point names the reference interface it replaces (paths relative to the Cerberus tree).
 * Return value: 0 on success, negative vilo_status on error (the reference's factors silently
 * `return true`, imu_leg_factor.cpp:385; numerical blow-ups only ROS_WARN, imu_factor.h:88-93).
 */
#ifndef VILO_GPU_H
#define VILO_GPU_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define VILO_WINDOW_SIZE 10           /* parameters.h:23 */
#define VILO_MAX_FRAMES 11            /* WINDOW_SIZE + 1 */
#define VILO_NUM_OF_F 1000            /* parameters.h:24 */
#define VILO_RESIDUAL_STATE_SIZE 31   /* parameters.h:103 */
#define VILO_NOISE_SIZE 46            /* parameters.h:104 */
#define VILO_MAX_PRIOR_BLOCKS 40
#define VILO_MAX_PRIOR_DIM 96         /* n <= 10*6 + 9 + 4 + 12 + 1 = 86 in the reference */

typedef enum {
  VILO_OK = 0,
  VILO_ERR_NO_DEVICE = -1,      /* no HIP device / extension cannot run: never falls back to CPU */
  VILO_ERR_BAD_ARG = -2,
  VILO_ERR_HIP = -3,
  VILO_ERR_NUMERIC = -4,        /* NaN/Inf or non-PD reduced system after mu escalation */
  VILO_ERR_UNSUPPORTED = -5
} vilo_status;

/* The reference's mutable config globals (src/utils/parameters.cpp:13-74) as one POD. */
typedef struct {
  double acc_n, acc_n_z, acc_w, gyr_n, gyr_w;
  double g_norm;
  double phi_n, dphi_n;
  double rho_c_n, rho_nc_n;
  double v_n_min_xy, v_n_min_z, v_n_min, v_n_max;
  double v_n_force_thres_ratio, v_n_term1_steep, v_n_term2_var_rescale, v_n_term3_distance_rescale;
  int32_t contact_sensor_type;
  int32_t pad0;
  double rho_fix[4][4];   /* per leg [ox, oy, d, lt]   (estimator.cpp:142-163) */
  double p_br[3];         /* estimator.cpp:140 */
  double R_br[9];         /* row-major, estimator.cpp:141 */
  double focal_length;    /* FOCAL_LENGTH, parameters.h:22; Projection*Factor::sqrt_info = f/1.5 I (estimator.cpp:124-126) */
  double huber_delta;     /* ceres::HuberLoss(1.0), estimator.cpp:1062 */
} vilo_config;

/* Values of config/a1_config/hardware_a1_vilo_config.yaml. */
void vilo_default_config(vilo_config *cfg);

/* One sample of IMULegIntegrationBase::push_back (imu_leg_integration_base.h:33-34): 35 doubles. */
typedef struct {
  double dt;
  double acc[3], gyr[3];
  double phi[12], dphi[12];
  double c[4];
} vilo_sample;

/* Public state of an IMULegIntegrationBase (imu_leg_integration_base.h:73-84). */
typedef struct {
  double sum_dt;
  double delta_p[3];
  double delta_q[4];      /* x y z w */
  double delta_v[3];
  double delta_eps[12];
  double lin_ba[3], lin_bg[3], lin_rho[4];
  double jacobian[31 * 31];    /* row-major */
  double covariance[31 * 31];  /* row-major */
} vilo_preint;

/* Public state of an IntegrationBase (integration_base.h:201-220). */
typedef struct {
  double sum_dt;
  double delta_p[3];
  double delta_q[4];
  double delta_v[3];
  double lin_ba[3], lin_bg[3];
  double jacobian[15 * 15];
  double covariance[15 * 15];
} vilo_preint_imu;

/* Parameter-block ids replace the raw addresses MarginalizationInfo keys on
 * (marginalization_factor.cpp:98-117, estimator.cpp:1358-1370): id = kind*16 + index. */
#define VILO_BLK_POSE 0
#define VILO_BLK_SB 1
#define VILO_BLK_LB 2
#define VILO_BLK_EX 3
#define VILO_BLK_TD 4
#define VILO_BLK_FEAT 5

/* MarginalizationInfo's product (marginalization_factor.h:57-82): the prior consumed by
 * MarginalizationFactor::Evaluate (marginalization_factor.cpp:347-395). */
typedef struct {
  int32_t n;                                  /* residuals = kept local dimension */
  int32_t n_blocks;
  int32_t block_id[VILO_MAX_PRIOR_BLOCKS];    /* after addr_shift */
  int32_t block_size[VILO_MAX_PRIOR_BLOCKS];  /* keep_block_size (global) */
  int32_t block_idx[VILO_MAX_PRIOR_BLOCKS];   /* keep_block_idx - m */
  double *x0;                                 /* keep_block_data, concatenated */
  double *J0;                                 /* linearized_jacobians, n x n row-major */
  double *r0;                                 /* linearized_residuals */
  int32_t valid;
  int32_t pad;
} vilo_prior;

/* What Estimator::optimization() reads (estimator.h:139-205 + f_manager.feature), flattened. */
typedef struct {
  int32_t n_frames;     /* frame_count + 1 */
  int32_t n_landmarks;  /* features with used_num >= 4 in list order (feature_manager.cpp:179-195) */
  int32_t n_obs;
  int32_t use_leg;      /* 1: IMULegFactor (estimator.cpp:1114-1159), 0: IMUFactor (:1160-1171) */
  const int32_t *lm_start_frame;   /* [L] FeaturePerId::start_frame */
  const int32_t *lm_obs_offset;    /* [L+1] into obs; a landmark's observations are consecutive frames */
  const double *obs;               /* [n_obs][11] FeaturePerFrame: point3 pointRight3 velocity2 velocityRight2 cur_td */
  const uint8_t *obs_is_stereo;    /* [n_obs] */
  const vilo_preint *preint;          /* [n_frames-1] il_pre_integrations[i+1] */
  const vilo_preint_imu *preint_imu;  /* [n_frames-1] pre_integrations[i+1] (use_leg == 0) */
  const vilo_prior *prior;            /* last_marginalization_info; NULL or !valid: none */
  int32_t leg_bias_const, ex_const, td_const;   /* SetParameterBlockConstant, estimator.cpp:1074-1105 */
  int32_t pad;
} vilo_window_desc;

/* para_Pose / para_SpeedBias / para_LegBias / para_Ex_Pose / para_Td / para_Feature
 * (estimator.h:189-196) in the layouts of vector2double (estimator.cpp:848-901). */
typedef struct {
  double *pose;        /* [n_frames][7]  px py pz qx qy qz qw */
  double *speed_bias;  /* [n_frames][9]  v ba bg */
  double *leg_bias;    /* [n_frames][4]  rho FL FR RL RR */
  double *ex_pose;     /* [2][7] */
  double *td;          /* [1] */
  double *inv_depth;   /* [L] */
} vilo_window_state;

/* ceres::Solver::Options as set at estimator.cpp:1221-1233 plus the Ceres 1.14 defaults in play. */
typedef struct {
  int32_t max_num_iterations;      /* NUM_ITERATIONS = 12 */
  int32_t fixed_iterations;        /* 1: no tolerance-based early exit (reproducible work; bench/parity) */
  double initial_trust_region_radius, max_trust_region_radius, min_trust_region_radius;
  double min_relative_decrease;
  double function_tolerance, gradient_tolerance, parameter_tolerance;
  double min_lm_diagonal, max_lm_diagonal;
  int32_t jacobi_scaling;
  int32_t max_solver_time_us;  /* Solver::Options::max_solver_time_in_seconds (estimator.cpp:1226-1233: SOLVER_TIME = 0.1 s, x 0.8 on MARGIN_OLD) as a
                                * device-clock budget in microseconds, checked per window where Ceres checks it (before an iteration starts);
                                * when spent the window ends with termination NO_CONVERGENCE. 0 (default): no budget — a solve takes ~3 ms.
                                * This field took the place of a former `reserved` int: fill the struct with vilo_default_solve_opts() first
                                * (a negative value is rejected with VILO_ERR_BAD_ARG) */
} vilo_solve_opts;
void vilo_default_solve_opts(vilo_solve_opts *o);

/* ceres::Solver::Summary subset. */
typedef struct {
  int32_t iterations, num_successful, termination /* 0 no_convergence, 1 convergence, 2 failure */, pad;
  double initial_cost, final_cost;
  double cost_trace[64];
  double radius_trace[64];
} vilo_solve_summary;

typedef struct vilo_ctx vilo_ctx;      /* one per host thread / GPU; owns device buffers and one HIP stream */
typedef struct vilo_batch vilo_batch;  /* device-resident batch of independent windows */

/* Replaces Estimator::setParameter (estimator.cpp:112-174) for the solver side. device = HIP ordinal. */
int vilo_create(vilo_ctx **ctx, const vilo_config *cfg, int device);
void vilo_destroy(vilo_ctx *ctx);
/* HIP devices this process sees (0 without a usable device): the "host thread per GPU" form of SURVEY 8(e) creates one context per ordinal
 * below it, each used from its own thread (tests/host_check/multi_device_check.cpp). */
int vilo_device_count(void);
const char *vilo_last_error(const vilo_ctx *ctx);

/* ---- ceres::CostFunction-shaped batched factor evaluation (host pointers) ------------------------
 * Semantics of CostFunction::Evaluate(double const* const* parameters, double* residuals, double** jacobians):
 * for factor f of n, parameter block k is params_k[f * size_k .. ]; residuals r[f * num_res ..];
 * jac_k, if non-NULL, receives row-major num_res x size_k per factor (global sizes, 7th pose column = 0).
 * obs: [n][12] = pts_i(3) pts_j(3) vel_i(2) vel_j(2) td_i td_j (Projection*Factor constructor arguments). */
/* ProjectionTwoFrameOneCamFactor::Evaluate <2,7,7,7,1,1>  projectionTwoFrameOneCamFactor.cpp:43-150 */
int vilo_eval_proj2f1c(vilo_ctx *ctx, int n, const double *obs, const double *pose_i, const double *pose_j,
                       const double *ex0, const double *inv_dep, const double *td, double *r, double *J_pose_i,
                       double *J_pose_j, double *J_ex0, double *J_feat, double *J_td);
/* ProjectionTwoFrameTwoCamFactor::Evaluate <2,7,7,7,7,1,1>  projectionTwoFrameTwoCamFactor.cpp:43-166 */
int vilo_eval_proj2f2c(vilo_ctx *ctx, int n, const double *obs, const double *pose_i, const double *pose_j,
                       const double *ex0, const double *ex1, const double *inv_dep, const double *td, double *r,
                       double *J_pose_i, double *J_pose_j, double *J_ex0, double *J_ex1, double *J_feat, double *J_td);
/* ProjectionOneFrameTwoCamFactor::Evaluate <2,7,7,1,1>  projectionOneFrameTwoCamFactor.cpp:42-134 */
int vilo_eval_proj1f2c(vilo_ctx *ctx, int n, const double *obs, const double *ex0, const double *ex1,
                       const double *inv_dep, const double *td, double *r, double *J_ex0, double *J_ex1,
                       double *J_feat, double *J_td);
/* IMULegFactor::Evaluate <31,7,9,4,7,9,4>  imu_leg_factor.cpp:173-386 */
int vilo_eval_imu_leg(vilo_ctx *ctx, int n, const vilo_preint *pre, const double *pose_i, const double *sb_i,
                      const double *lb_i, const double *pose_j, const double *sb_j, const double *lb_j, double *r,
                      double *J_pose_i, double *J_sb_i, double *J_lb_i, double *J_pose_j, double *J_sb_j, double *J_lb_j);
/* IMUFactor::Evaluate <15,7,9,7,9>  imu_factor.h:28-188 */
int vilo_eval_imu(vilo_ctx *ctx, int n, const vilo_preint_imu *pre, const double *pose_i, const double *sb_i,
                  const double *pose_j, const double *sb_j, double *r, double *J_pose_i, double *J_sb_i,
                  double *J_pose_j, double *J_sb_j);
/* MarginalizationFactor::Evaluate  marginalization_factor.cpp:347-395. params: concatenated kept blocks in
 * prior order, n_eval evaluations back to back; J (optional): n x sum(block_size) row-major per evaluation. */
int vilo_eval_prior(vilo_ctx *ctx, int n_eval, const vilo_prior *prior, const double *params, double *r, double *J);
/* PoseLocalParameterization::Plus  pose_local_parameterization.cpp:12-27 (batched) */
int vilo_pose_plus(vilo_ctx *ctx, int n, const double *x, const double *delta, double *x_plus_delta);
/* ceres::HuberLoss::Evaluate (used at marginalization_factor.cpp:53) — host-side helper */
void vilo_huber(double delta, double s, double rho[3]);

/* ---- IMULegIntegrationBase(ctor) + push_back/repropagate  imu_leg_integration_base.cpp:7-136 ---------
 * Interval i integrates samples[offsets[i] .. offsets[i+1]): the first sample of the range plays the
 * constructor's (acc_0, gyr_0, phi_0, dphi_0, c_0) (its dt is ignored), the rest are push_back()ed.
 * lin: [n][10] = ba(3) bg(3) rho(4). */
int vilo_preintegrate(vilo_ctx *ctx, int n_intervals, const vilo_sample *samples, const int32_t *offsets,
                      const double *lin, vilo_preint *out);
/* IntegrationBase equivalent (integration_base.h:18-170); lin: [n][6] = ba bg. */
int vilo_preintegrate_imu(vilo_ctx *ctx, int n_intervals, const vilo_sample *samples, const int32_t *offsets,
                          const double *lin, vilo_preint_imu *out);

/* ---- the same objects kept on the device and updated as samples arrive: IMULegIntegrationBase::push_back per IMU/leg
 * message (Estimator::processIMULeg, estimator.cpp:619-626) instead of re-integrating an interval. A pool of n objects;
 * pushing an interval in pieces gives bitwise the result of vilo_preintegrate on the whole interval. ---------------------- */
typedef struct vilo_preint_streams vilo_preint_streams;
int vilo_preint_streams_create(vilo_ctx *ctx, int n, vilo_preint_streams **pool);
/* the same pool of IntegrationBase objects (integration_base.h) for USE_LEG = 0: reset takes lin [n][6] = ba bg, the leg fields
 * of the samples are ignored, vilo_preint_streams_read_imu returns their state */
int vilo_preint_streams_create_imu(vilo_ctx *ctx, int n, vilo_preint_streams **pool);
void vilo_preint_streams_destroy(vilo_ctx *ctx, vilo_preint_streams *pool);
/* new IMULegIntegrationBase{acc_0, gyr_0, phi_0, dphi_0, c_0, ba, bg, rho} (imu_leg_integration_base.cpp:7-42) for the
 * objects ids[0..n): first[k] holds the constructor's measurement, lin [n][10] = ba bg rho. ids must be distinct. */
int vilo_preint_streams_reset(vilo_ctx *ctx, vilo_preint_streams *pool, int n, const int32_t *ids, const vilo_sample *first,
                              const double *lin);
/* push_back (imu_leg_integration_base.cpp:44-60): object ids[k] receives samples[offsets[k] .. offsets[k+1]) in order. */
int vilo_preint_streams_push(vilo_ctx *ctx, vilo_preint_streams *pool, int n, const int32_t *ids, const vilo_sample *samples,
                             const int32_t *offsets);
/* the public state of the objects ids[0..n) (what IMULegFactor reads) */
int vilo_preint_streams_read(vilo_ctx *ctx, vilo_preint_streams *pool, int n, const int32_t *ids, vilo_preint *out);
int vilo_preint_streams_read_imu(vilo_ctx *ctx, vilo_preint_streams *pool, int n, const int32_t *ids, vilo_preint_imu *out);

/* ---- Estimator::optimization(), solve half (estimator.cpp:1054-1245) --------------------------------
 * Synchronous; n_windows = 1 reproduces the reference call. States are updated in place with the
 * solver result (double2vector's gauge fix is vilo_gauge_fix below). */
int vilo_solve_windows(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *inout,
                       const vilo_solve_opts *opts, vilo_solve_summary *out);
/* Many host windows in one vilo_solve_windows / vilo_optimize_windows call (from 2 * sub_windows up, and more than 256 of them with
 * landmarks: a call that as one batch takes the full batch's kernels) go through `lanes` internal contexts of the same device in
 * sub-batches, one host thread per lane, so that packing, the PCIe transfer and the solver work at the same time. The sub-batches run the
 * full batch's kernel set and the whole call's solver form whatever their size: the result is the one batch's bit for bit, and `inout` is
 * written only if every sub-batch came through. Default 4 lanes of 1024 windows (VILO_HOST_PIPELINE="lanes,sub_windows" at vilo_create);
 * lanes < 2 or sub_windows == 0: always one batch. */
int vilo_set_host_pipeline(vilo_ctx *ctx, int lanes, int sub_windows);

/* Device-resident form of the same call, for batches (independent windows: robots / replays / seeds). */
int vilo_batch_create(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *init,
                      vilo_batch **batch);
int vilo_batch_reset(vilo_ctx *ctx, vilo_batch *batch);  /* restore the uploaded initial states (device-side copy); the landmark mask and the snapshot slot stay as they are */
/* sqrt_info = LLT(cov^-1)^T of the batch's preintegration records again (asynchronous): vilo_batch_create runs it once; the reference
 * recomputes it in every IMULegFactor::Evaluate (imu_leg_factor.cpp:197-198), a caller that replays a resident batch can charge it per solve */
int vilo_batch_prepare(vilo_ctx *ctx, vilo_batch *batch);
/* BASELINE configs[2] ("K1 re-propagation of all 10 intervals inside the iteration"): hand the batch the samples behind its IMU-leg
 * records — samples [offsets[10 w + k], offsets[10 w + k + 1]) are interval k of window w, the first one the constructor sample
 * (IMULegIntegrationBase(acc_0, gyr_0, ...), imu_leg_integration_base.cpp:7-42), the rest its push_back()s; n_windows * 10 + 1 offsets,
 * empty ranges for intervals the window does not have. From then on vilo_batch_solve integrates every live interval again
 * (IMULegIntegrationBase::repropagate(Bai, Bgi, rhoi), imu_leg_integration_base.cpp:62-86) at the biases of every point it
 * linearises or evaluates, followed by the sqrt_info of the new covariance, and vilo_batch_marginalize does so at the accepted state.
 * samples == NULL switches it off again. The records the batch was built with are overwritten. */
int vilo_batch_set_samples(vilo_ctx *ctx, vilo_batch *batch, const vilo_sample *samples, const int32_t *offsets);
int vilo_batch_solve(vilo_ctx *ctx, vilo_batch *batch, const vilo_solve_opts *opts);
/* out[w] (optional) receives window w's current state: rows 0 .. n_frames - 1 of pose, speed_bias and leg_bias, both extrinsics, td and the
 * window's n_landmarks inverse depths. A window of fewer than 11 frames: the rows at and beyond n_frames of the caller's three per-frame
 * arrays are absent frames, which no kernel reads as state; the call does not write them, they stay bytewise what the caller left there. */
int vilo_batch_download(vilo_ctx *ctx, vilo_batch *batch, vilo_window_state *out, vilo_solve_summary *summaries);
void vilo_batch_destroy(vilo_ctx *ctx, vilo_batch *batch);
/* GPU time of the last vilo_batch_solve on ctx's stream (HIP events), and per-kernel-group breakdown. */
double vilo_last_solve_ms(const vilo_ctx *ctx);
/* Host wall time inside the last vilo_batch_create on ctx (what handing over HOST windows costs before the first kernel): out_ms[0] total,
 * [1] packing into the device layouts, [2] allocation + upload of observations / states / priors, [3] preintegration records up + their
 * sqrt_info; *bytes_up (optional): bytes moved to the device. vilo_last_download_ms: the same for the last vilo_batch_download. */
int vilo_last_create_ms(const vilo_ctx *ctx, double out_ms[4], double *bytes_up);
double vilo_last_download_ms(const vilo_ctx *ctx);

/* double2vector gauge fix (estimator.cpp:903-957): yaw/position re-anchoring of the solver output. */
int vilo_gauge_fix(vilo_ctx *ctx, int n_windows, const vilo_window_state *before, vilo_window_state *after, int n_frames);

/* ---- marginalisation half (estimator.cpp:1247-1455; MarginalizationInfo::{preMarginalize,marginalize,
 * getParameterBlocks} marginalization_factor.cpp:119-333). mode 0 = MARGIN_OLD, 1 = MARGIN_SECOND_NEW.
 * out->x0/J0/r0 must point at caller buffers of >= 7*VILO_MAX_PRIOR_BLOCKS, VILO_MAX_PRIOR_DIM^2, VILO_MAX_PRIOR_DIM doubles.
 * MARGIN_SECOND_NEW with a prior that does not hold para_Pose[WINDOW_SIZE-1] marginalises nothing and hands the
 * incoming prior back unchanged (estimator.cpp:1379-1380); without any prior out->valid = 0. */
int vilo_marginalize(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                     int mode, vilo_prior *out);
/* The same on a batch that is already resident, linearised at its device state (after vilo_batch_solve + vilo_batch_download; `state` is
 * the host copy of that state, `in` the descriptors the batch was created from). modes[w]: 0, 1 as above, < 0: leave window w alone.
 * With vilo_batch_set_samples in force the intervals are integrated again at the accepted state first. The call's device memory is
 * returned to the context's pool when it returns. The batch's states, uploaded copy, mask, snapshot and (without samples) records are
 * left as they were; the solve summaries are NOT kept: a vilo_batch_download after this call reports zeroed summaries, so read them
 * before it. */
int vilo_batch_marginalize(vilo_ctx *ctx, vilo_batch *batch, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                           const int *modes, vilo_prior *out);

/* ---- Estimator::optimization() as ONE call (estimator.cpp:1054-1458): solve, double2vector gauge fix, marginalisation
 * linearised at that result, all on one device-resident batch (one packing, no host round trip between the halves).
 * inout: states, replaced by the gauge-fixed result. marginalization_flag: [n_windows] 0 MARGIN_OLD / 1 MARGIN_SECOND_NEW
 * (estimator.h:64-68), or NULL to skip the marginalisation; windows with n_frames < WINDOW_SIZE + 1 are not marginalised
 * (estimator.cpp:1243) and their next_prior entry is left untouched. next_prior: [n_windows], buffers as for vilo_marginalize. */
int vilo_optimize_windows(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *inout,
                          const vilo_solve_opts *opts, const int *marginalization_flag, vilo_prior *next_prior,
                          vilo_solve_summary *summaries);

/* ---- device-resident hand-over between frames ("a device-resident prior") ----------------------------
 * last_marginalization_info objects kept in HBM: slot = {n, kept blocks, keep_block_data on the host; linearized_jacobians and
 * linearized_residuals on the device}. A window then names the slot its prior comes from and the slot the next prior goes to,
 * and the preintegration objects (vilo_preint_streams) its IMU factors read, instead of carrying 74 KB of J0 and 156 KB of
 * records through host memory in both directions every frame. */
typedef struct vilo_prior_pool vilo_prior_pool;
int vilo_prior_pool_create(vilo_ctx *ctx, int n_slots, vilo_prior_pool **pool);
void vilo_prior_pool_destroy(vilo_ctx *ctx, vilo_prior_pool *pool);
int vilo_prior_pool_upload(vilo_ctx *ctx, vilo_prior_pool *pool, int slot, const vilo_prior *prior);   /* NULL / !valid: empties the slot */
int vilo_prior_pool_download(vilo_ctx *ctx, vilo_prior_pool *pool, int slot, vilo_prior *out);        /* buffers as for vilo_marginalize */
int vilo_prior_pool_dim(const vilo_prior_pool *pool, int slot);   /* n of the slot, 0: no prior */

typedef struct {
  vilo_preint_streams *preint_pool;   /* NULL: the window's vilo_window_desc::preint records are used */
  const int32_t *preint_ids;          /* [n_frames - 1] object of interval k (frames k -> k+1) */
  const double *preint_sum_dt;        /* [n_frames - 1] their sum_dt, host side (intervals above 10 s carry no factor, estimator.cpp:1118) */
  vilo_prior_pool *prior_pool;        /* NULL: vilo_window_desc::prior / the next_prior argument are used */
  int32_t prior_slot;                 /* < 0: no prior */
  int32_t next_prior_slot;            /* where vilo_optimize_windows_resident leaves the new last_marginalization_info */
} vilo_resident_refs;

/* vilo_optimize_windows with per-window device handles (refs[w]); next_prior may be NULL when every window names a prior pool. */
int vilo_optimize_windows_resident(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_resident_refs *refs,
                                   vilo_window_state *inout, const vilo_solve_opts *opts, const int *marginalization_flag,
                                   vilo_prior *next_prior, vilo_solve_summary *summaries);

/* GPU time (HIP events on ctx's stream) of the kernels of the last vilo_marginalize: linearisation + marginalisation. */
double vilo_last_marginalize_ms(const vilo_ctx *ctx);

/* ---- state covariance of a window (no counterpart in the reference: Cerberus publishes odometry with a zero covariance) ----------
 * Definition. At the window's current state, H = J^T J is the Gauss-Newton Hessian of the solve's problem: Ceres' evaluator Jacobian
 * (whitened, HuberLoss' Corrector applied to the visual blocks), without LM damping and without Jacobi scaling, in the local coordinates of
 * PoseLocalParameterization (dp in the world frame, dtheta the body-frame right perturbation q (x) dq(dtheta)). Constant blocks are left
 * out as the solve leaves them out (ex_const, td_const, leg_bias_const; the leg biases when use_leg == 0). The inverse depths are
 * eliminated; their variances are not an output.
 *   VILO_COV_GAUGE_FRAME0 (default): Sigma = N (N^T H N)^-1 N^T, N a basis of the tangent space with frame 0's dp = 0 and
 *     (R0^T e_z) . dtheta0 = 0: the covariance conditioned on frame 0's position and world yaw, the four quantities double2vector
 *     resets (vilo_gauge_fix). It does not depend on the choice of N; frame 0's position rows are zero, its rotation block has rank 2.
 *   VILO_COV_GAUGE_NONE: Sigma = H^-1, meaningful only where the prior fixes the gauge.
 * Rank deficiency: the landmarks are eliminated first; the reduced camera-side system (restricted to N under FRAME0) is scaled to unit
 * diagonal and factored, speed / bias chain first, then the 79-wide pose system. A window whose inputs are not finite or one of whose
 * pivots is not above min_reciprocal_condition (Ceres' Covariance::Options default 1e-14) gets status 1 and NaN in all its outputs
 * (Covariance::Compute returning false); the other windows are unaffected.
 * Outputs, per window w:
 *   frames [W][VILO_MAX_FRAMES][19][19]  diagonal block of each frame in the order dp dtheta v ba bg rho, with the pose <-> speed-bias <->
 *                                        rho cross terms; zero for absent frames (n_frames < 11) and constant blocks
 *   poses  [W][79][79]  (want_poses)     joint covariance of the 11 poses (66), ex0 ex1 (12) and td (1); rows of constant / absent blocks zero
 *   status [W]                           0 OK, 1 rank deficient / not finite, 2 window invalid (a preintegration covariance without
 *                                        sqrt_info: the window the solve fails with termination FAILURE); NaN outputs for 1 and 2
 * The covariance is that of the state the batch holds when the call is made: the solver's state right after vilo_batch_solve,
 * double2vector's re-anchored one once vilo_batch_gauge_fix has run on the batch. The fix rotates the window by a yaw and shifts it, and
 * Sigma is not transported through that rotation here: to have the covariance at the re-anchored state, fix first and query then
 * (a host-side vilo_gauge_fix of downloaded states does not change what the batch holds). */
#define VILO_COV_GAUGE_FRAME0 0
#define VILO_COV_GAUGE_NONE 1
typedef struct {
  int32_t gauge;                     /* VILO_COV_GAUGE_* */
  int32_t pad0;
  double min_reciprocal_condition;   /* pivot threshold of the equilibrated system (default 1e-14) */
  int32_t want_poses;                /* 1: fill `poses` (then it must not be NULL) */
  int32_t pad1;
} vilo_cov_opts;
void vilo_default_cov_opts(vilo_cov_opts *o);
/* At the batch's device state, normally right after vilo_batch_solve. Leaves the batch as it was: states, candidate, prior, trust-region
 * state and the summaries vilo_batch_download reports; a following vilo_batch_solve gives what it gives without this call. Its device
 * memory is returned when the call returns. opts NULL: vilo_default_cov_opts. Bad arguments: VILO_ERR_BAD_ARG. */
int vilo_batch_covariance(vilo_ctx *ctx, vilo_batch *batch, const vilo_cov_opts *opts, double *frames, double *poses, int32_t *status);
/* The same for host windows at the given states (e.g. an Estimator after optimization()): one batch is created and destroyed. */
int vilo_window_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_cov_opts *opts,
                           double *frames, double *poses, int32_t *status);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_covariance or vilo_batch_landmark_covariance: linearisation + covariance
 * kernels, without the copies out. */
double vilo_last_covariance_ms(const vilo_ctx *ctx);

/* ---- landmark covariance: inverse depths and world points (pubPointCloud's cloud with its uncertainty) -------------------------------
 * Same problem, gauge and conventions as the state covariance above (H = J^T J at the batch's current state, undamped and unscaled, Huber
 * corrector applied; FRAME0 or NONE; constant blocks left out). Sigma_PP is what `poses` holds: unscaled, original basis, zero rows for
 * constant, absent and gauge-held dimensions. For landmark l of a window with start frame s, first observation f (obs[lm_obs_offset[l]][0:3]),
 * inverse depth rho, E = H_ll and w = H_{P,l} (79 entries; a landmark couples to poses, extrinsics and td only):
 *   inv_depth_var   Sigma_rr = 1/E + w^T Sigma_PP w / E^2   (and Sigma_rP = -w^T Sigma_PP / E)
 *   points          p = R_s (R_c f / rho + t_c) + P_s        ((P_s, R_s): pose s of the solver state, (t_c, R_c): ex_pose[0])
 *   point_cov       Sigma_p = J Sigma_13 J^T (3 x 3), Sigma_13 the joint covariance of [dp_s dtheta_s dt_c dtheta_c rho] (Sigma_PP's dims
 *                   6s..6s+5 and 66..71, Sigma_rP, Sigma_rr) and J the derivative in PoseLocalParameterization's local coordinates:
 *                   d/ddp_s = I, d/ddtheta_s = -R_s [R_c f/rho + t_c]x, d/ddt_c = R_s, d/ddtheta_c = -R_s R_c [f/rho]x,
 *                   d/drho = -R_s R_c f / rho^2 (with ex_const the extrinsic rows of Sigma_PP are zero and drop out).
 * These are the landmark rows of the full inverse with the landmarks kept: N (N^T H_full N)^-1 N^T, or H_full^-1 under NONE. Like the frame
 * blocks they belong to the state the batch holds when the call is made: the solver's, or double2vector's re-anchored one after
 * vilo_batch_gauge_fix. A window with status 1 or 2 gets NaN for all its
 * landmarks; the other windows are unaffected. Landmarks' cross-covariances with each other are not an output.
 * Outputs: landmarks concatenated window by window, inside a window in the caller's vilo_window_desc order (sum L = total landmarks):
 *   inv_depth_var [sum L], points [sum L][3], point_cov [sum L][3][3], status [W];
 *   frames, poses: as vilo_batch_covariance returns them (bit for bit), or NULL to leave them out. opts->want_poses is ignored: a non-NULL
 *   `poses` decides. The landmark buffers may be NULL only when the batch has no landmarks. Bad arguments: VILO_ERR_BAD_ARG.
 * The batch is left as vilo_batch_covariance leaves it; its device memory is likewise returned when the call returns. */
int vilo_batch_landmark_covariance(vilo_ctx *ctx, vilo_batch *batch, const vilo_cov_opts *opts, double *frames, double *poses, double *inv_depth_var,
                                   double *points, double *point_cov, int32_t *status);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_landmark_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_cov_opts *opts,
                                    double *frames, double *poses, double *inv_depth_var, double *points, double *point_cov, int32_t *status);

/* ---- residuals at the current state (Ceres Problem::Evaluate's residuals; Estimator::outliersRejection, estimator.cpp:1741-1798) ----
 * State: the batch's current state, what vilo_batch_download returns (inverse depths included): the initial state before any solve or after
 * vilo_batch_reset, the accepted state after a solve, double2vector's re-anchored one after vilo_batch_gauge_fix: whichever of them the caller last
 * produced (reprojection errors and the factors' costs do not depend on that choice: the gauge fix moves every frame by the same rigid
 * transform; a prior's residual does, it holds the poses it was linearised at).
 * Costs: Ceres' 1/2 sum rho(|r|^2) over the problem the solve builds, in the units of vilo_solve_summary::final_cost. The IMU-leg / IMU factor
 * counts its whitened residual; the three projection factors use sqrt_info = focal_length / 1.5, td compensation and the HuberLoss; the prior
 * is MarginalizationFactor::Evaluate's. Constant blocks change no cost. With vilo_batch_set_samples in force the IMU factors are evaluated on
 * records integrated again at the current state, as vilo_batch_marginalize does (into buffers of the call's own: the batch's records and
 * contact-force filters are not touched).
 * Per landmark (concatenated window by window, inside a window in the caller's vilo_window_desc order, as vilo_batch_landmark_covariance):
 *   lm_cost       1/2 sum rho over the landmark's residual blocks;
 *   lm_reproj_px  (err / cnt) * focal_length, err and cnt exactly the sum and count of Estimator::reprojectionError in outliersRejection:
 *                 frame by frame from the start frame, the left-camera term first (not on the start frame), then the right-camera term of
 *                 every stereo observation (the start frame included); no td compensation, no velocities, depth = 1 / inv_depth, ex_pose[0]
 *                 for the start frame and ex_pose[c] for the observing camera c;
 *   lm_flags      bit 0: (err / cnt) * focal_length > outlier_threshold_px (the set outliersRejection hands to removeOutlier);
 *                 bit 1: 1 / inv_depth < 0 (setDepth's solve_flag = 2, dropped by removeFailures);
 *                 bit 2: at least one of the landmark's blocks is in Huber's linear region (|r|^2 > huber_delta^2).
 * Per observation (obs_residuals rows follow the caller's obs rows, concatenated by window; a window without landmarks has none):
 *   [0:2] the left camera's whitened residual (ProjectionTwoFrameOneCamFactor against the start frame), [2:4] the right camera's
 *   (ProjectionTwoFrameTwoCamFactor, or ProjectionOneFrameTwoCamFactor on the start frame): the values Evaluate returns, before the loss.
 *   A pair is NaN where no block exists: the left pair of the start frame, the right pair of a mono observation.
 * Per interval (imu_residuals [W][10][31]): the factor's whitened residual; use_leg == 0: entries 15..30 are zero. Intervals without a factor
 *   are zero; the intervals of a status-2 window whose record has no sqrt_info are NaN.
 * Side effects: none on the batch's states, candidate, trust-region state, summaries or what a following solve computes (the guarantee of
 * vilo_batch_covariance). The call's device memory is returned when it returns; the table of the landmarks' observation rows is uploaded
 * at the first call and kept with the batch.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx, batch or windows, a threshold that is negative or not finite, n_windows < 1. */
typedef struct {
  double outlier_threshold_px;   /* 3.0: ave_err * FOCAL_LENGTH > 3 (estimator.cpp:1796) */
} vilo_residual_opts;
void vilo_default_residual_opts(vilo_residual_opts *o);

typedef struct {
  double cost;               /* prior_cost + sum(imu_cost) + visual_cost, in the units of vilo_solve_summary::final_cost */
  double prior_cost;         /* 0 without a prior */
  double imu_cost[10];       /* interval k (frames k -> k+1); 0 where the window has no factor (absent frame, sum_dt > 10 s) */
  double visual_cost;        /* with the HuberLoss, as the solver counts it */
  double visual_cost_plain;  /* the same residual blocks without the loss */
  int32_t n_visual_blocks;   /* residual blocks of the three projection factors */
  int32_t n_huber_active;    /* of which |r|^2 > huber_delta^2 (down-weighted) */
  int32_t n_outliers;        /* landmarks with flag bit 0 */
  int32_t n_negative_depth;  /* landmarks with flag bit 1 */
  int32_t status;            /* 0 OK; 2 window invalid (a record without sqrt_info): its imu_cost entries for those intervals and cost are NaN */
  int32_t pad;
} vilo_window_residual;

/* windows [W] is required; every other output may be NULL to leave it out:
 *   lm_cost, lm_reproj_px [sum L] doubles, lm_flags [sum L] bytes, obs_residuals [sum n_obs][4], imu_residuals [W][10][31].
 * opts NULL: vilo_default_residual_opts. */
int vilo_batch_residuals(vilo_ctx *ctx, vilo_batch *batch, const vilo_residual_opts *opts, vilo_window_residual *windows, double *lm_cost,
                         double *lm_reproj_px, uint8_t *lm_flags, double *obs_residuals, double *imu_residuals);
/* The same for host windows at the given states: one batch is created, reported once and destroyed. */
int vilo_window_residuals(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                          const vilo_residual_opts *opts, vilo_window_residual *windows, double *lm_cost, double *lm_reproj_px,
                          uint8_t *lm_flags, double *obs_residuals, double *imu_residuals);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_residuals: its kernels (and, with samples in force, the re-integration),
 * without the copies out. */
double vilo_last_residuals_ms(const vilo_ctx *ctx);

/* ---- landmark mask of a resident batch (Estimator::processImage's f_manager.removeOutlier(removeIndex), estimator.cpp:812-814;
 *      FeatureManager::removeOutlier) ----
 * Takes landmarks out of a resident batch on the device, without a new batch: while a mask is in force the batch behaves as a batch built
 * from the same windows with the masked landmarks deleted — in vilo_batch_solve, vilo_batch_download, vilo_batch_residuals and
 * vilo_batch_marginalize. solve -> residuals -> mask(outliers) -> solve, or -> marginalize, run on one batch with no host round trip.
 * How: the call clears the valid bits of the masked landmarks' observations in the batch's flag image (the kernels above skip an
 * observation without one, as they skip the tail of a short track); the image as uploaded is kept in a second copy, allocated with the mask
 * at the first mask call (2 - 3 KB per window at 200 landmarks; a batch that is never masked holds nothing more than before).
 * source   VILO_MASK_GIVEN          mask_in [sum L] bytes, non-zero = masked (concatenated window by window, inside a window in the caller's
 *                                   vilo_window_desc order, as vilo_batch_triangulate's mask);
 *          VILO_MASK_OUTLIER_FLAGS  vilo_batch_residuals' landmark test run inside this call at the batch's current state (and current
 *                                   mask): the landmarks whose lm_flags byte intersects flag_bits (default 3: bit 0, what outliersRejection
 *                                   hands to removeOutlier, and bit 1, what setDepth / removeFailures reject), at outlier_threshold_px;
 *                                   byte for byte (vilo_batch_residuals' lm_flags & flag_bits) != 0 of the same batch. A landmark that is
 *                                   already masked has no reprojection error (its bit 0 is clear): accumulate rounds with VILO_MASK_OR;
 *          VILO_MASK_CLEAR          no landmark: removes the mask and restores the flag image bit for bit (combine is not read).
 * combine  VILO_MASK_REPLACE the selection becomes the mask; VILO_MASK_OR it is added to the mask in force.
 * A masked landmark: no residual block, nothing in cost, gradient, pose system or prior; its step is exactly zero, so its inverse depth
 * comes back from the solve bitwise as it went in; vilo_batch_residuals reports lm_cost 0, no blocks, flag bit 0 clear, lm_reproj_px
 * NaN (0 / 0 observations) and every obs_residuals row of the landmark NaN (no block exists); flag bit 1 is a property of the inverse depth alone, so a masked landmark whose inverse depth is negative keeps
 * it and is counted in n_negative_depth. The free-running solve's ParameterToleranceReached test still counts its inverse depth in |x| (fixed-iteration
 * solves have no such test).
 * The mask persists across vilo_batch_reset (which restores every inverse depth, masked ones included, to the uploaded values),
 * vilo_batch_prepare, repeated solves and replays of the captured launch sequence; only this call changes it. Without a mask call, and
 * after VILO_MASK_CLEAR, every call gives bitwise what it gave before this call existed.
 * The other calls on a resident batch, while at least one landmark is masked:
 *   honour the mask   vilo_batch_solve, _download, _residuals, _marginalize (a masked landmark that starts at frame 0 is left out of the
 *                     eliminated set, as the deleted one is: no detour through the eigen path);
 *   do not read landmarks   vilo_batch_gauge_fix, _failure_detection, _gyro_bias_align, _dead_reckon, _dead_reckon_covariance, _repropagate, _set_samples, _prepare, _reset;
 *   refuse            vilo_batch_covariance, _landmark_covariance, _gradient, _triangulate, _frame_pose_pnp, _predict_next_frame return
 *                     VILO_ERR_UNSUPPORTED with vilo_last_error saying so; they work again after VILO_MASK_CLEAR (or a mask that selects nothing).
 * records [W] (optional): status VILO_MASK_OK, or VILO_MASK_NO_LANDMARKS for a window left without a landmark (not an error: it solves as
 * prior plus IMU factors); n_landmarks; n_masked now; n_newly_masked by this call; n_obs_left: valid observations of the unmasked landmarks.
 * mask_out [sum L] (optional): the mask in force after the call, caller order. Mask and records do not depend on the batch a window shares
 * or on its position.
 * A mask call that fails with VILO_ERR_HIP after its kernels were launched leaves the mask in force unknown: vilo_batch_solve, _residuals,
 * _marginalize and the refusing calls then fail, with vilo_last_error saying so, until a mask call has gone through.
 * A batch without landmarks: VILO_OK, no array is touched. Bad arguments (VILO_ERR_BAD_ARG): NULL ctx or batch, an unknown source or
 * combine, VILO_MASK_GIVEN without mask_in, a threshold that is negative or not finite; n_windows < 1 in the host-window form. */
#define VILO_MASK_GIVEN 0
#define VILO_MASK_OUTLIER_FLAGS 1
#define VILO_MASK_CLEAR 2
#define VILO_MASK_REPLACE 0
#define VILO_MASK_OR 1
#define VILO_MASK_OK 0
#define VILO_MASK_NO_LANDMARKS 1
typedef struct {
  int32_t source;                /* VILO_MASK_GIVEN */
  int32_t combine;               /* VILO_MASK_REPLACE */
  uint32_t flag_bits;            /* 3 (OUTLIER_FLAGS) */
  int32_t pad;
  double outlier_threshold_px;   /* 3.0 (OUTLIER_FLAGS) */
} vilo_mask_opts;
void vilo_default_mask_opts(vilo_mask_opts *o);
typedef struct {
  int32_t status;           /* VILO_MASK_OK, VILO_MASK_NO_LANDMARKS */
  int32_t n_landmarks;
  int32_t n_masked;         /* landmarks masked after the call */
  int32_t n_newly_masked;   /* of which were not masked before it */
  int32_t n_obs_left;       /* valid observations of the landmarks that are not masked */
  int32_t pad;
} vilo_window_mask_record;
/* opts NULL: vilo_default_mask_opts (GIVEN, REPLACE). */
int vilo_batch_mask_landmarks(vilo_ctx *ctx, vilo_batch *batch, const vilo_mask_opts *opts, const uint8_t *mask_in, uint8_t *mask_out,
                              vilo_window_mask_record *records);
/* The same for host windows at the given states: one batch is created, masked, reported and destroyed (mask_out and records are what the
 * call is for: the selection of the device's outlier test, and its counts). */
int vilo_window_mask_landmarks(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                               const vilo_mask_opts *opts, const uint8_t *mask_in, uint8_t *mask_out, vilo_window_mask_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_mask_landmarks: its kernels, without the copies in and out. */
double vilo_last_mask_ms(const vilo_ctx *ctx);

/* ---- cost gradient and Gauss-Newton diagonal at the current state (Ceres Problem::Evaluate's gradient) ----
 * Definition. At the batch's current state, the one vilo_batch_download returns (inverse depths included), over the residual blocks of the
 * problem the solve builds:
 *   g = sum_blocks rho'(s) J^T r        the gradient of the cost vilo_batch_residuals reports,
 *   h = sum_blocks rho'(s) diag(J^T J)  the diagonal of the Gauss-Newton Hessian,
 * in the local coordinates of PoseLocalParameterization (dp, dtheta on the 7-dimensional blocks), undamped and without Jacobi scaling, r and
 * J whitened as the factors return them, the HuberLoss applied to the visual blocks as Ceres' Corrector applies it (first branch, rho'' <= 0:
 * residual and Jacobian times sqrt(rho')). It is the same H whose inverse vilo_batch_covariance returns (VILO_COV_GAUGE_NONE; the landmarks
 * kept), so state_diag is that matrix's diagonal, and g_i / sqrt(h_i) is dimensionless.
 * With vilo_batch_set_samples in force the call does what vilo_batch_covariance does: the linearisation pass both share integrates the
 * batch's own records again at the current state first, in place, as vilo_batch_marginalize does (an interval already integrated at these
 * biases is kept as it is).
 * Layouts. state_grad, state_diag [W][222] in the tangent form of vector2double's order: pose 11 x 6 (dp dtheta), speed-bias 11 x 9
 * (v ba bg), leg bias 11 x 4, extrinsics 2 x 6 (dt dtheta), td 1. Constant blocks (ex_const, td_const, leg_bias_const; the leg biases when
 * use_leg == 0) and absent frames (n_frames < 11) are zero in both and not counted in the record. lm_grad, lm_diag [sum L]: the inverse
 * depths, concatenated window by window, inside a window in the caller's vilo_window_desc order (as vilo_batch_landmark_covariance).
 * The record's norms run over the free local coordinates, inverse depths included. max_norm is the quantity the solve's
 * gradient_tolerance test reads (Ceres' gradient_max_norm: unscaled, over exactly this set; the solver forms sum in other orders and
 * agree with it to rounding). The arg-max is the first entry of the largest |g_i| in the order state_grad, then lm_grad.
 * A window of status 2 gets NaN in its norms and all its array entries (n_free 0, arg-max -1); the other windows are unaffected. Status 1
 * leaves the arrays as computed, with NaN norms and arg-max -1.
 * Side effects: vilo_batch_covariance's. It leaves the batch as it was: states, candidate, prior, trust-region state and the summaries
 * vilo_batch_download reports; a following vilo_batch_solve gives what it gives without this call. Its device memory is returned when the
 * call returns. Every output of a window is bitwise independent of the batch it shares and of its position in it.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx, batch or windows, n_windows < 1. */
typedef struct {
  double max_norm;          /* max |g_i| over the free local coordinates, inverse depths included */
  double norm;              /* sqrt(sum g_i^2) over the same set */
  double scaled_max;        /* max |g_i| / sqrt(h_i) over entries with h_i > 0 (dimensionless) */
  int32_t argmax_kind;      /* of max_norm: VILO_BLK_* 0 pose, 1 speed-bias, 2 leg bias, 3 extrinsic, 4 td; 5 inverse depth */
  int32_t argmax_index;     /* frame / camera index, or the landmark's index in the caller's order */
  int32_t argmax_component; /* local coordinate inside the block */
  int32_t n_free;           /* number of free local coordinates counted */
  int32_t status;           /* 0 OK; 1 an input or a sum is not finite; 2 window invalid (a record without sqrt_info), as vilo_batch_residuals */
  int32_t pad;
} vilo_window_gradient_record;   /* 48 bytes (a C typedef cannot share the name of the function vilo_window_gradient) */

/* windows [W] is required; state_grad, state_diag, lm_grad, lm_diag may each be NULL to leave it out. */
int vilo_batch_gradient(vilo_ctx *ctx, vilo_batch *batch, vilo_window_gradient_record *windows, double *state_grad, double *state_diag,
                        double *lm_grad, double *lm_diag);
/* The same for host windows at the given states: one batch is created, reported once and destroyed. */
int vilo_window_gradient(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                         vilo_window_gradient_record *windows, double *state_grad, double *state_diag, double *lm_grad, double *lm_diag);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_gradient: linearisation + k_gradient, without the copies out. */
double vilo_last_gradient_ms(const vilo_ctx *ctx);

/* ---- Gauss-Newton / damped step at the current state (the linear system of Ceres 1.14's dogleg and Levenberg-Marquardt strategies) ----
 * Definition. State and problem as for the cost gradient above: g and H = sum_blocks rho'(s) J^T J are exactly vilo_batch_gradient's and
 * vilo_batch_covariance's (whitened, Huber corrector applied, PoseLocalParameterization's local coordinates; constant blocks and absent
 * frames left out; the inverse depths part of the system). With h = diag(H), what state_diag / lm_diag report:
 *   s_i   = 1 / (1 + sqrt(h_i))                                   Ceres' Jacobi scale,
 *   D^2_i = clamp(s_i^2 h_i, min_lm_diagonal, max_lm_diagonal),
 *   delta = s o y,  (S H S + mu diag(D^2)) y = -S g,  S = diag(s),
 * which is (H + mu diag(D^2_i / s_i^2)) delta = -g: the Gauss-Newton system the solver forms build (mu = 0: the plain Gauss-Newton step).
 * The inverse depths are eliminated first, with E~_l = E_l + mu D^2_l / s_l^2, and their step is returned.
 * Gauge (opts->gauge, VILO_COV_GAUGE_*). NONE solves the full system: meaningful only where a prior or mu > 0 fixes it. FRAME0 restricts
 * the step to frame 0's dp = 0 and (R_0^T e_z) . dtheta_0 = 0: delta = N z with N^T (H + mu diag(D^2 / s^2)) N z = -N^T g, N the
 * orthonormal basis vilo_batch_covariance uses ([e1 e2 u], u = R_0^T e_z, on frame 0's rotation); those four directions of the step are zero.
 * mu [W], or NULL for 0. A window whose mu is negative or not finite gets status 1.
 * Outputs. state_step [W][222], lm_step [sum L]: exactly state_grad's / lm_grad's layouts, so that they go straight into
 * vilo_batch_retract; entries of constant blocks, absent frames and gauge-held directions are zero. The record:
 *   model_cost_change = -(g^T delta + delta^T H delta / 2) with the undamped H (= -g^T delta / 2 + mu sum_i (D^2_i / s_i^2) delta_i^2 / 2),
 *   scaled_norm = |D o y|, the quantity the dogleg compares with the trust-region radius,  norm = |delta|,  grad_dot_step = g^T delta,
 *   n_free: the coordinates solved for (vilo_batch_gradient's n_free, less 4 under FRAME0).
 * Status 0 OK; 1 an input is not finite, or a pivot of the equilibrated system (unit diagonal) is at or below min_pivot: every output of
 * the window is NaN, the other windows are untouched; 2 window invalid (a record without sqrt_info), as vilo_batch_gradient.
 * Side effects: vilo_batch_gradient's — the SolverStates are copied aside and back, records are integrated again in place when samples are
 * in force, a following vilo_batch_solve is bitwise what it would have been. While a landmark is masked the call returns
 * VILO_ERR_UNSUPPORTED. Its device memory is returned when the call returns. Every output of a window is bitwise independent of the batch
 * it shares and of its position in it. Bad arguments (VILO_ERR_BAD_ARG): NULL ctx, batch or windows, an unknown gauge, pad0 != 0, diagonal
 * bounds that are negative, unordered or not finite, a negative or non-finite min_pivot, n_windows < 1. */
typedef struct {
  int32_t gauge;                           /* VILO_COV_GAUGE_* */
  int32_t pad0;                            /* 0 */
  double min_lm_diagonal, max_lm_diagonal; /* the clamp of D^2 (Ceres: 1e-6, 1e32) */
  double min_pivot;                        /* smallest accepted Cholesky pivot of the equilibrated system */
} vilo_step_opts;   /* 32 bytes */
/* VILO_COV_GAUGE_NONE (what the solver solves), 1e-6, 1e32, 1e-14 */
void vilo_default_step_opts(vilo_step_opts *o);
typedef struct {
  double model_cost_change, scaled_norm, norm, grad_dot_step;
  int32_t n_free, status;
} vilo_window_step_record;   /* 40 bytes */
/* windows [W] is required; state_step and lm_step may each be NULL to leave it out. opts NULL: vilo_default_step_opts. */
int vilo_batch_gauss_newton_step(vilo_ctx *ctx, vilo_batch *batch, const vilo_step_opts *opts, const double *mu,
                                 vilo_window_step_record *windows, double *state_step, double *lm_step);
/* The same for host windows at the given states: one batch is created, queried once and destroyed. */
int vilo_window_gauss_newton_step(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                  const vilo_step_opts *opts, const double *mu, vilo_window_step_record *windows, double *state_step,
                                  double *lm_step);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_gauss_newton_step: linearisation + k_gn_step, without the copies. */
double vilo_last_gn_step_ms(const vilo_ctx *ctx);
/* The kernel form of vilo_batch_gauss_newton_step on this context: 0 (default) streams the 143 x 80 coupling through per-call global memory,
 * two workgroups per CU; 1 keeps it in LDS, one workgroup per CU. The same definition and bounds; the two differ in rounding only (the split
 * of the landmark passes). Kept for measurement (tools/time_gn_step.py). VILO_ERR_BAD_ARG for any other value. */
int vilo_set_gn_step_form(vilo_ctx *ctx, int form);

/* ---- dogleg trust-region step at the current state (Ceres 1.14's DoglegStrategy, TRADITIONAL_DOGLEG: the step vilo_batch_solve takes
 * inside its kernels, opened to a caller who runs the trust-region loop with an acceptance rule of their own: one iteration is
 * vilo_batch_dogleg_step -> vilo_batch_trial_cost -> vilo_batch_retract on one resident batch, with one linearisation) ----
 * Definition. g, H, h = diag H, s_i = 1 / (1 + sqrt(h_i)) and D^2_i = clamp(s_i^2 h_i, min_lm_diagonal, max_lm_diagonal) are
 * vilo_batch_gauss_newton_step's. Put S = diag(s). For window w with trust-region radius Delta = radius[w] and mu = mu[w]:
 *   scaled gradient       g^ = (S g) / D
 *   Cauchy point          u = g^ / D,  alpha = g^T g^ / (u^T S H S u)
 *   Gauss-Newton point    p^_gn = D o y with (S H S + mu D^2) y = -S g: bitwise what vilo_batch_gauss_newton_step solves at the same mu,
 *                         gauge and kernel form (vilo_set_gn_step_form); the inverse depths are eliminated and their part is returned
 *   branch 0, |p^_gn| <= Delta:            p^ = p^_gn
 *   branch 1, alpha |g^| >= Delta:         p^ = -(Delta / |g^|) g^
 *   branch 2, otherwise:                   p^ = -alpha (1 - beta) g^ + beta p^_gn, the point of the segment from the Cauchy point a =
 *       -alpha g^ to b = p^_gn at distance Delta, by Ceres' two-case formula: with c = a.(b - a) and d = sqrt(c^2 + |b - a|^2 (Delta^2 - |a|^2)),
 *       beta = (d - c) / |b - a|^2 if c <= 0, else (Delta^2 - |a|^2) / (d + c)
 *   step                  delta = s o (p^ / D)
 * Gauge (opts->gauge). NONE: as above. FRAME0: the problem restricted to vilo_batch_gauss_newton_step's subspace delta = N z (frame 0's
 * dp = 0 and (R_0^T e_z) . dtheta_0 = 0). With M = diag(D^2 / s^2), the metric in which |p^| is measured (|p^|^2 = delta^T M delta), the
 * Cauchy direction is M's steepest descent inside the subspace, S u = N (N^T M N)^-1 N^T g (which is g / M on every coordinate but frame
 * 0's pose), |g^|^2 = g^T S u, and the rest reads the same; the four held directions of the step are zero.
 * Outputs. state_step [W][222], lm_step [sum L]: delta in state_grad's / lm_grad's layouts, so that it goes straight into
 * vilo_batch_retract and vilo_batch_trial_cost; entries of constant blocks, absent frames and gauge-held directions are zero. On branch 0
 * they are bitwise vilo_batch_gauss_newton_step's. cauchy_state / cauchy_lm (optional, each may be NULL): -alpha s o (g^ / D), the Cauchy
 * point in the same layouts. The record: see the struct; model_cost_change = -(g^T delta + delta^T H delta / 2) with the undamped H (by
 * bilinearity from H [S u | delta_gn], no third product), the quantity TrustRegionMinimizer divides the cost decrease by and whose sign
 * decides whether the step is valid.
 * radius [W] is required; mu [W], or NULL for 0. Status 0 OK; 1 as vilo_batch_gauss_newton_step (an input or a sum that is not finite, a
 * pivot at or below min_pivot, a mu that is negative or not finite), or a radius that is <= 0 or not finite: every output of the window is
 * NaN (branch -1), the other windows are untouched; 2 window invalid (a record without sqrt_info): NaN.
 * Side effects, samples in force, masked batches (VILO_ERR_UNSUPPORTED), per-call device memory: vilo_batch_gauss_newton_step's. Every
 * output of a window is bitwise independent of the batch it shares and of its position in it. Bad arguments (VILO_ERR_BAD_ARG): NULL ctx,
 * batch, windows or radius, and vilo_step_opts' conditions on the options, n_windows < 1. */
typedef struct {
  int32_t gauge;                           /* VILO_COV_GAUGE_* */
  int32_t pad0;                            /* 0 */
  double min_lm_diagonal, max_lm_diagonal; /* the clamp of D^2 (Ceres: 1e-6, 1e32) */
  double min_pivot;                        /* smallest accepted Cholesky pivot of the equilibrated Gauss-Newton system */
} vilo_dogleg_opts;   /* 32 bytes: vilo_step_opts' fields and defaults */
/* VILO_COV_GAUGE_NONE (what the solver solves), 1e-6, 1e32, 1e-14 */
void vilo_default_dogleg_opts(vilo_dogleg_opts *o);
typedef struct {
  double alpha;               /* Cauchy step length in the D-scaled space */
  double gradient_norm;       /* |g^| */
  double gauss_newton_norm;   /* |D o y|: vilo_batch_gauss_newton_step's scaled_norm, bitwise */
  double step_norm;           /* |p^|: what DoglegStrategy::StepAccepted multiplies by 3 (the radius itself on branch 1) */
  double beta;                /* interpolation weight; 1 on the Gauss-Newton branch, 0 on the Cauchy branch */
  double model_cost_change;   /* -(g^T delta + delta^T H delta / 2), undamped H */
  double grad_dot_step, norm; /* g^T delta, |delta| */
  int32_t branch;             /* 0 Gauss-Newton inside the radius, 1 Cauchy-limited, 2 interpolated; -1 with a status other than 0 */
  int32_t n_free, status, pad;/* n_free: vilo_batch_gauss_newton_step's */
} vilo_window_dogleg_record;   /* 80 bytes */
/* windows [W] and radius [W] are required; state_step, lm_step, cauchy_state and cauchy_lm may each be NULL to leave it out. opts NULL:
 * vilo_default_dogleg_opts. */
int vilo_batch_dogleg_step(vilo_ctx *ctx, vilo_batch *batch, const vilo_dogleg_opts *opts, const double *radius, const double *mu,
                           vilo_window_dogleg_record *windows, double *state_step, double *lm_step, double *cauchy_state, double *cauchy_lm);
/* The same for host windows at the given states: one batch is created, queried once and destroyed. */
int vilo_window_dogleg_step(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                            const vilo_dogleg_opts *opts, const double *radius, const double *mu, vilo_window_dogleg_record *windows,
                            double *state_step, double *lm_step, double *cauchy_state, double *cauchy_lm);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_dogleg_step: linearisation + k_gn_step + k_dogleg, without the copies. */
double vilo_last_dogleg_step_ms(const vilo_ctx *ctx);

/* ---- Gauss-Newton Hessian-vector products at the current state (what a Cauchy point, a predicted decrease of a caller's own step, the
 * curvature along a search direction, conjugate gradients or a few Lanczos steps need) ----
 * Definition. State and problem as for the cost gradient above: g and H = sum_blocks rho'(s) J^T J are exactly vilo_batch_gradient's,
 * vilo_batch_covariance's and vilo_batch_gauss_newton_step's (whitened, Huber corrector applied, PoseLocalParameterization's local
 * coordinates; constant blocks and absent frames left out; the inverse depths part of the system: not eliminated, not damped, no gauge).
 * For every window w and each of its K = n_vec vectors v_k over the 222 state coordinates and the window's L_w inverse depths:
 *   y_k = H v_k,   record[w][k]: vHv = v_k^T H v_k,  g_dot_v = g^T v_k,  model_cost_change = -g_dot_v - vHv / 2,  status.
 * Layouts. state_vec, state_out [W][K][222]: every row in state_grad's layout. lm_vec, lm_out [K sum L]: window w's block starts at
 * K * (sum of L of the windows before it); vector k starts at k * L_w inside it, in the caller's vilo_window_desc order. records [W][K].
 * state_vec or lm_vec NULL: zero; state_out or lm_out NULL: not wanted. K is the same for all windows, 1 <= K <= VILO_HV_MAX_VECTORS (16:
 * the K vectors are the columns of one 16-column matrix-core tile, and one pass over the landmarks' coupling rows serves them all).
 * Entries of v on constant blocks (ex_const, td_const, leg_bias_const; the leg biases when use_leg == 0) and on absent frames are not
 * read — NaN there is harmless — and the outputs at those entries are 0.
 * Status per (window, vector): 0 OK; 1 a read entry of v_k (or a sum) is not finite: that vector's outputs (at the entries that are
 * read) and record are NaN, the window's other vectors and the other windows are untouched; 2 window invalid (a record without sqrt_info), as vilo_batch_gradient: NaN.
 * Side effects: vilo_batch_gradient's — the SolverStates are copied aside and back, records are integrated again in place when samples are
 * in force, a following vilo_batch_solve is bitwise what it would have been. While a landmark is masked the call returns
 * VILO_ERR_UNSUPPORTED. Its device memory is returned when the call returns. Every output of a (window, vector) pair is bitwise
 * independent of the batch it shares and of its position in it, and of K and of k: column 0 of a K = 5 call is the K = 1 call on that vector.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx, batch or records, n_vec out of range, n_windows < 1. */
#define VILO_HV_MAX_VECTORS 16
typedef struct {
  double vHv, g_dot_v, model_cost_change;
  int32_t status, pad;
} vilo_hess_vec_record;   /* 32 bytes */
int vilo_batch_hessian_vector(vilo_ctx *ctx, vilo_batch *batch, int n_vec, const double *state_vec, const double *lm_vec,
                              vilo_hess_vec_record *records, double *state_out, double *lm_out);
/* The same for host windows at the given states: one batch is created, queried once and destroyed. */
int vilo_window_hessian_vector(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, int n_vec,
                               const double *state_vec, const double *lm_vec, vilo_hess_vec_record *records, double *state_out, double *lm_out);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_hessian_vector: linearisation + k_hess_vec, without the copies. */
double vilo_last_hess_vec_ms(const vilo_ctx *ctx);

/* ---- the cost at up to 16 trial steps from the current state, without moving it (the actual decrease of a trust-region gain ratio, a
 * backtracking line search, a ladder of damped steps; TrustRegionMinimizer's candidate evaluation opened to the caller) ----
 * Definition. For every window w and each of its K = n_steps steps delta_k the trial state is x_k = x [+] alpha[w][k] * delta_k, exactly
 * vilo_batch_retract with base CURRENT: s = alpha * delta rounded once, x + s rounded once, pose and extrinsic blocks through
 * vilo_pose_plus — the two calls run one device function. The same coordinates are not read (constant blocks, absent frames, masked
 * landmarks): NaN there is harmless. records[w][k] holds the costs vilo_batch_residuals would report at x_k: visual_cost, the sum of its
 * ten imu_cost, prior_cost (k_accept's normal-equation form), and cost, their sum in that call's order (prior, intervals 0 .. 9, visual);
 * cost_change = base cost - cost; n_negative_depth counts the unmasked landmarks whose trial inverse depth is < 0.
 * base (optional) [W]: the same record at x itself — x as it stands, not a zero-step retract, which would normalise the quaternions
 * again — with cost_change 0. best (optional) [W]: the smallest k of status OK with the lowest cost among those with cost_change > 0, or -1.
 * Layouts, as vilo_batch_hessian_vector: state_step [W][K][222], every row in state_grad's layout; lm_step [K sum L], window w's block at
 * K * (sum of L of the windows before it), step k at k * L_w inside it, in the caller's vilo_window_desc order; alpha [W][K] or NULL for
 * 1; records [W][K]. state_step or lm_step NULL: zero. Masked landmarks (vilo_batch_mask_landmarks) are honoured as vilo_batch_residuals
 * and vilo_batch_retract honour them: they contribute nothing and their steps are not read.
 * Status per (window, step): OK; NUMERIC alpha or a read entry of the step is not finite: the record's doubles are NaN, its counts 0, the
 * window's other steps and the other windows are untouched; INVALID a live preintegration record of the window has no sqrt_info (as
 * vilo_batch_residuals' status 2): imu_cost, cost and cost_change are NaN, in base too; NOT_FINITE the step is finite, the cost at the
 * trial state is not: the values as computed.
 * No side effects: current and uploaded state, snapshot slot, records, mask, solve summaries and SolverStates are not written; a
 * vilo_batch_solve after the call is bit for bit the solve without it. With vilo_batch_set_samples in force the call returns
 * VILO_ERR_UNSUPPORTED and writes nothing (K re-integrations at K bias sets are another matter). Its device memory is returned when the
 * call returns. Every record is bitwise independent of the batch the window shares, of its position in it, of K and of k: column 0 of
 * a K = 5 call is the K = 1 call on that step. No floating-point atomics; every sum has a fixed order.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing written): NULL ctx, batch or records, n_steps outside 1 .. VILO_TRIAL_MAX_STEPS, n_windows < 1. */
#define VILO_TRIAL_MAX_STEPS 16
#define VILO_TRIAL_OK 0
#define VILO_TRIAL_NUMERIC 1      /* alpha or a read entry of the step not finite: record NaN */
#define VILO_TRIAL_INVALID 2      /* a live record of the window has no sqrt_info (as vilo_batch_residuals' status 2): NaN */
#define VILO_TRIAL_NOT_FINITE 3   /* the step is finite, the cost at the trial state is not: the values as computed */
typedef struct {
  double cost, visual_cost, imu_cost, prior_cost;   /* as vilo_window_residual's, at the trial state; imu_cost = the sum over the intervals */
  double cost_change;                               /* base cost - cost: positive = the step lowers the cost */
  int32_t n_negative_depth, status;                 /* unmasked landmarks whose trial inverse depth is < 0; VILO_TRIAL_* */
} vilo_trial_record;   /* 48 bytes */
int vilo_batch_trial_cost(vilo_ctx *ctx, vilo_batch *batch, int n_steps, const double *state_step, const double *lm_step,
                          const double *alpha, vilo_trial_record *base, vilo_trial_record *records, int32_t *best);
/* The same for host windows at the given states: one batch is created, queried once and destroyed. */
int vilo_window_trial_cost(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, int n_steps,
                           const double *state_step, const double *lm_step, const double *alpha, vilo_trial_record *base,
                           vilo_trial_record *records, int32_t *best);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_trial_cost: its four kernels, without the copies. */
double vilo_last_trial_cost_ms(const vilo_ctx *ctx);

/* ---- landmark depths from the current poses (FeatureManager::triangulate, feature_manager.cpp:302-382 with triangulatePoint :198-212; the
 * arithmetic of FeatureManager::removeBackShiftDepth :450-479) ----
 * State: the batch's current state, what vilo_batch_download returns. Rotation matrices are taken from the normalised quaternions, as
 * vilo_batch_residuals' reprojection error takes them. Per landmark, concatenated window by window, inside a window in the caller's
 * vilo_window_desc order (as vilo_batch_landmark_covariance):
 *   depth  a selected landmark: localPoint.z() of the reference's branch if it is positive, else init_depth. The stereo branch applies when
 *          opts->stereo is set and the landmark's first observation is stereo: left and right camera of the start frame ([R0^T | -R0^T t0] as
 *          :312-325 forms it), the first observation's point and pointRight. Otherwise the left camera of the start frame and of the next
 *          frame, with the first two observations' point. The point is the right singular vector of the smallest singular value of
 *          triangulatePoint's 4 x 4 design matrix. (The reference's multi-view branch below :383 is not reachable for a landmark with two
 *          observations and is not built; a landmark with a single mono observation is never selected.)
 *          An unselected landmark: 1 / inv_depth of the current state, unchanged.
 *   flags  bit 0: selected; bit 1: the stereo branch was taken; bit 2: the init_depth fallback was taken (localPoint.z() not positive);
 *          bit 3: localPoint.z() is not finite.
 *   shift_inv_depth (optional)  removeBackShiftDepth on the inverse depth the call leaves (after the write-back when opts->write is set): for a
 *          landmark with start frame 0, pts_j = new_R^T (marg_R (point / inv_depth) + marg_P - new_P) with the marg pose the left camera of
 *          frame 0 and the new pose the left camera of frame 1: 1 / pts_j.z if that is positive, else 1 / init_depth. Every other landmark:
 *          its inverse depth, unchanged. Erasing tracks and shifting start frames stays with the host's feature window.
 * opts->select: VILO_TRI_UNSET the landmarks whose inverse depth is not positive (the reference's `estimated_depth > 0` test), VILO_TRI_ALL every
 * landmark, VILO_TRI_MASK those with mask[l] != 0 (mask [sum L], same order as the outputs).
 * Side effects: with opts->write == 0 none (the guarantee of vilo_batch_residuals). With opts->write == 1 the current inverse depth of every
 * selected landmark becomes 1 / depth and nothing else changes: not the uploaded initial state vilo_batch_reset restores, not the camera-side
 * state, the records or the prior; a following vilo_batch_solve starts from the new values. The call's device memory is returned when it
 * returns. Every output of a landmark is bitwise independent of the batch its window shares and of the window's position in it.
 * A batch without landmarks: VILO_OK, the arrays are not touched. flags and shift_inv_depth may be NULL to leave them out; opts NULL:
 * vilo_default_triangulate_opts.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx or batch, NULL depth with landmarks present, VILO_TRI_MASK without a mask, an unknown select,
 * init_depth not finite or not positive. */
#define VILO_TRI_UNSET 0
#define VILO_TRI_ALL 1
#define VILO_TRI_MASK 2
typedef struct {
  double init_depth;   /* INIT_DEPTH, 5.0 (hardware_a1_vilo_config.yaml) */
  int32_t stereo;      /* STEREO, 1 */
  int32_t select;      /* VILO_TRI_* */
  int32_t write;       /* 1: the batch's current inverse depth of every selected landmark becomes 1 / depth */
  int32_t pad;
} vilo_triangulate_opts;
void vilo_default_triangulate_opts(vilo_triangulate_opts *o);

int vilo_batch_triangulate(vilo_ctx *ctx, vilo_batch *batch, const vilo_triangulate_opts *opts, const uint8_t *mask, double *depth,
                           uint8_t *flags, double *shift_inv_depth);
/* The same for host windows at the given states: one batch is created and destroyed; with opts->write the new inverse depths are written
 * into state[w].inv_depth. */
int vilo_window_triangulate(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                            const vilo_triangulate_opts *opts, const uint8_t *mask, double *depth, uint8_t *flags, double *shift_inv_depth);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_triangulate: k_triangulate, without the copies. */
double vilo_last_triangulate_ms(const vilo_ctx *ctx);

/* ---- frame pose by PnP from the landmarks that have depth (FeatureManager::initFramePoseByPnP, feature_manager.cpp:259-300, with
 * solvePoseByPnP :215-257) ----
 * State: the batch's current state, what vilo_batch_download returns. Rotation matrices are taken from the normalised quaternions, as
 * vilo_batch_triangulate takes them. Per window, for one frame k with 1 <= k <= n_frames - 1 (opts->frame; -1: the window's last frame):
 *   points   landmark l is used when its current inverse depth is > 0 and 1 <= k - start_l < n_obs_l. World point
 *            Rs[s] (ric0 (point_0 / inv_depth) + tic0) + Ps[s] with s = start_l (:273-274); image point: point.xy of observation k - s, no td
 *            compensation, as in the reference.
 *            Deviation 1: k - s = 0 is left out. In the reference's call order such a landmark has no depth yet; here it would define the
 *            pose by itself. Deviation 2: everything stays FP64 (the reference rounds to cv::Point2f / Point3f).
 *   start    VILO_PNP_GUESS_PREVIOUS (the reference): RCam = Rs[k-1] ric0, PCam = Rs[k-1] tic0 + Ps[k-1]; VILO_PNP_GUESS_CURRENT: the same of
 *            frame k's own pose. Either is inverted to cam_T_w = (R, t) as :222-223 does.
 *   iterate  plain Gauss-Newton on sum |pi(R X + t) - uv|^2 with K = I and no distortion: left-multiplicative perturbation (dtheta, dt) on
 *            cam_T_w (R <- Exp(dtheta) R, t <- Exp(dtheta) t + dt), the 6 x 6 normal system solved by Cholesky; stops when |delta| <=
 *            opts->step_tolerance, at the latest after opts->max_iterations steps (20: the count cv::solvePnP's iterative mode runs at
 *            most). This is the library's own restatement: cv::solvePnP's Levenberg-Marquardt stops at FLT_EPSILON; parity is unpinned
 *            against OpenCV.
 *   result   Rs[k] = RCam ric0^T, Ps[k] = -RCam ric0^T tic0 + PCam (:292-293) with (RCam, PCam) the inverse of (R, t), written as
 *            pose[w] = [px py pz qx qy qz qw], the quaternion normalised, qw >= 0.
 * records[w] (may be NULL): final_cost = 1/2 sum r^2 at the pose returned, initial_cost the same at the start, n_points, iterations (steps
 * taken) and status:
 *   VILO_PNP_OK                 the last step was within the tolerance
 *   VILO_PNP_NOT_ENOUGH_POINTS  fewer than four points (:226)
 *   VILO_PNP_NO_CONVERGENCE     max_iterations steps, the last above the tolerance; pose is the last iterate
 *   VILO_PNP_NUMERIC            a Cholesky pivot not positive, a value not finite, or a point with camera-frame z <= 0 at an iterate
 *   VILO_PNP_NO_FRAME           k out of range for this window
 * For any status but OK and NO_CONVERGENCE pose[w] is frame k's current pose bit for bit (the reference leaves the pose alone when PnP
 * fails; NO_FRAME: row k of the padded state) and the costs are those of the last evaluation made, 0 if none was.
 * Side effects: with opts->write == 0 none. With opts->write == 1 frame k's pose in the batch's current state becomes pose[w] for the
 * windows with status OK and nothing else changes: vilo_batch_reset still restores the uploaded state; a following
 * vilo_batch_triangulate or vilo_batch_solve (plain launches or the captured graph) starts from the new pose. The call's device memory is
 * returned when it returns. Every output of a window is bitwise independent of the batch it shares and of its position in it.
 * opts NULL: vilo_default_pnp_opts.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx or batch, NULL pose with windows present, an unknown guess, frame below -1, 0 or above
 * VILO_MAX_FRAMES - 1, max_iterations below 1 or above 64, step_tolerance not finite or negative. */
#define VILO_PNP_GUESS_PREVIOUS 0
#define VILO_PNP_GUESS_CURRENT 1
#define VILO_PNP_OK 0
#define VILO_PNP_NOT_ENOUGH_POINTS 1
#define VILO_PNP_NO_CONVERGENCE 2
#define VILO_PNP_NUMERIC 3
#define VILO_PNP_NO_FRAME 4
typedef struct {
  int32_t frame;            /* -1: the window's last frame */
  int32_t guess;            /* VILO_PNP_GUESS_* */
  int32_t write;            /* 1: frame k's pose of the batch's current state becomes the result (status OK only) */
  int32_t max_iterations;   /* 20 */
  double step_tolerance;    /* 1e-12 */
} vilo_pnp_opts;
void vilo_default_pnp_opts(vilo_pnp_opts *o);
typedef struct {
  double final_cost;
  double initial_cost;
  int32_t n_points;
  int32_t iterations;
  int32_t status;           /* VILO_PNP_* */
  int32_t pad;
} vilo_window_pnp_record;

int vilo_batch_frame_pose_pnp(vilo_ctx *ctx, vilo_batch *batch, const vilo_pnp_opts *opts, double *pose, vilo_window_pnp_record *records);
/* The same for host windows at the given states: one batch is created and destroyed; with opts->write the new pose row is written into
 * state[w].pose. */
int vilo_window_frame_pose_pnp(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_pnp_opts *opts,
                               double *pose, vilo_window_pnp_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_frame_pose_pnp: k_frame_pose_pnp, without the copies. */
double vilo_last_pnp_ms(const vilo_ctx *ctx);

/* ---- gyroscope-bias alignment of a window's preintegrated rotations with its poses (solveGyroscopeBias,
 * src/initial/initial_aligment.cpp:14-40; called by processImage once the window fills, estimator.cpp:738-762) ----
 * State: the batch's current state, what vilo_batch_download returns. Quaternions are normalised, as vilo_batch_triangulate and
 * vilo_batch_frame_pose_pnp normalise them. Per window, over EVERY interval k, 0 <= k < n_frames - 1, whether or not it carries a factor
 * (the reference walks all of all_image_frame; sum_dt > 10 s does not exclude an interval):
 *   q_ij   q_k^-1 (x) q_{k+1}, from the poses (:30 takes it from the rotation matrices, so its w is >= 0 whatever the sign of the stored
 *          quaternions; see r_k).
 *   J_k    the 3 x 3 block d(rotation) / d(gyro bias) of interval k's record Jacobian (:31): rows 3.., columns 24.. of the 31 x 31
 *          IMU-leg record (ILO_R, ILO_BG, parameters.h:138,145) when use_leg == 1, rows 3.., columns 12.. of the 15 x 15 IMU record
 *          (O_R, O_BG, parameters.h:121,124) when use_leg == 0. It is the block the IMU factors call dq_dbg.
 *   gamma  opts->linearization == VILO_GYRO_RECORD (default; the reference, literally): the record's delta_q.
 *          VILO_GYRO_CORRECTED: delta_q (x) deltaQ(J_k (Bg_k - lin_bg_k)), the corrected rotation the IMU factors use
 *          (imu_leg_factor.cpp / imu_factor.h: corrected_delta_q), Bg_k frame k's gyro bias of the current state. The two coincide when
 *          the state's biases are the records' linearisation point, as they are at the reference's call; the corrected form makes the call
 *          meaningful on a batch whose biases have moved, and makes repeated calls with write-back converge.
 *   r_k    2 vec(gamma^-1 (x) q_ij) (:32), gamma^-1 the conjugate over the squared norm (Eigen's inverse()), the product negated when its
 *          w is < 0: q and -q are the same rotation, and pose quaternions of neighbouring frames loaded from another source may lie in
 *          opposite hemispheres. Where they do not (vector2double's output), nothing is negated and the bits are the reference's formula's.
 *   step   A = sum J_k^T J_k, b = sum J_k^T r_k (:33-34), delta_bg = A^-1 b by an UNPIVOTED LDL^T of the symmetric 3 x 3. Eigen's ldlt()
 *          (:36) pivots; the two agree to rounding (A is a sum of squares of blocks close to -sum_dt I).
 * Outputs per window: delta_bg[w][3], and records[w] (may be NULL): initial_cost = 1/2 sum |r_k|^2, model_cost = 1/2 sum |r_k - J_k delta_bg|^2,
 * n_intervals = n_frames - 1 and status:
 *   VILO_GYRO_OK
 *   VILO_GYRO_NO_INTERVALS  n_frames < 2 (vilo_batch_create refuses such a window: not reachable through a batch created by this library)
 *   VILO_GYRO_SINGULAR      an LDL^T pivot is <= 0 (e.g. every J_k zero)
 *   VILO_GYRO_NUMERIC       a sum, a pivot or the step is not finite
 * For any status but OK delta_bg is 0 and model_cost is initial_cost (NaN where a residual is not finite).
 * Side effects: with opts->write == 0 none. With opts->write == 1, for the windows with status OK, Bg_i += delta_bg for EVERY frame
 * i < n_frames of the batch's current state (:39-40: one IEEE addition per component) and nothing else changes: vilo_batch_reset still
 * restores the uploaded state; a following vilo_batch_solve (plain launches or the captured graph) starts from the new biases.
 * The reference's trailing repropagate loops (:42-47, estimator.cpp:752-760) are not part of this call: vilo_batch_repropagate (below) is
 * that loop, once, at chosen biases (VILO_REPROP_POINT_STARTUP: estimator.cpp:752-760 literally). Without it the batch's records
 * keep their linearisation point and the factors' first-order correction takes the new bias; with vilo_batch_set_samples in force the
 * next solve integrates every interval again at the new biases anyway.
 * With samples in force the records in device memory may sit at a rejected candidate point, so the call first integrates them again at
 * the current state, on copies of its own, as vilo_batch_residuals does (intervals above 10 s, which carry no factor, keep the record they
 * have): the batch's records and contact-force filters are not touched, and both linearizations then return the same bits.
 * The call's device memory is returned when it returns. Every output of a window is bitwise independent of the batch it shares and of
 * its position in it. opts NULL: vilo_default_gyro_opts.
 * Bad arguments (VILO_ERR_BAD_ARG): NULL ctx or batch, NULL delta_bg with windows present, an unknown linearization, write other than 0
 * or 1. A batch that holds no preintegration records on the device: VILO_ERR_UNSUPPORTED. A batch without windows: VILO_OK, nothing is
 * written. */
#define VILO_GYRO_RECORD 0
#define VILO_GYRO_CORRECTED 1
#define VILO_GYRO_OK 0
#define VILO_GYRO_NO_INTERVALS 1
#define VILO_GYRO_SINGULAR 2
#define VILO_GYRO_NUMERIC 3
typedef struct {
  int32_t linearization;    /* VILO_GYRO_RECORD / VILO_GYRO_CORRECTED */
  int32_t write;            /* 1: Bg of every frame of the batch's current state += delta_bg (status OK only) */
} vilo_gyro_opts;
void vilo_default_gyro_opts(vilo_gyro_opts *o);
typedef struct {
  double initial_cost;
  double model_cost;
  int32_t n_intervals;
  int32_t status;           /* VILO_GYRO_* */
} vilo_window_gyro_record;

int vilo_batch_gyro_bias_align(vilo_ctx *ctx, vilo_batch *batch, const vilo_gyro_opts *opts, double *delta_bg, vilo_window_gyro_record *records);
/* The same for host windows at the given states: one batch is created and destroyed; with opts->write the new biases are written into
 * state[w].speed_bias. */
int vilo_window_gyro_bias_align(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_gyro_opts *opts,
                                double *delta_bg, vilo_window_gyro_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_gyro_bias_align: k_gyro_bias_align and, with samples in force, the
 * re-integration before it, without the copies out. */
double vilo_last_gyro_align_ms(const vilo_ctx *ctx);

/* ---- where the landmarks will be in the next frame's cameras (Estimator::predictPtsInNextFrame, estimator.cpp:1694-1727; called by
 * processImage after the solve and the outlier rejection, :811-819) ----
 * State: the batch's current state, what vilo_batch_download returns. Rotation matrices are taken from the normalised quaternions, as
 * vilo_batch_triangulate takes them. Per window, with k = n_frames - 1 (the reference's frame_count):
 *   next pose  opts->mode == VILO_PREDICT_CONSTANT_VELOCITY (default; the reference, :1700-1703): nextT = curT (prevT^-1 curT) with curT the
 *              pose of frame k and prevT that of frame k - 1, written as
 *                P_n = P_k + R_k R_{k-1}^T (P_k - P_{k-1}),   q_n = normalise(q_k (x) q_{k-1}^-1 (x) q_k)
 *              on the normalised pose quaternions, with no change of hemisphere.
 *              VILO_PREDICT_GIVEN: P_n, q_n = next_pose_in[w] = [px py pz qx qy qz qw], the quaternion normalised by the call: a caller that
 *              dead-reckons the pose of the frame to come from IMU and leg odometry (processIMULeg) has something better than constant
 *              velocity.
 *              In both modes R_n is the rotation matrix of q_n normalised (once more, in the constant-velocity mode): everything after the
 *              next pose is one code path, and VILO_PREDICT_GIVEN with the next_pose a constant-velocity call returned gives that call's
 *              points and flags bit for bit.
 *   selection  (:1708-1713) landmark l is predicted when its current inverse depth is > 0, it has at least two observations and its track
 *              ends at the last frame: start_l + n_obs_l - 1 == k. The batch holds the tracks the solve uses; the reference also predicts
 *              tracks too short for the solve.
 *   point      (:1715-1719) pts_j = ric0 (point_0 (1 / inv_depth)) + tic0, point_0 the first observation's point; pts_w = R_s pts_j + P_s
 *              with s = start_l; pts_local = R_n^T (pts_w - P_n); pts_cam = ric0^T (pts_local - tic0). With pts_cam_right given, the same
 *              with ric1, tic1 in the last step: where a stereo tracker searches in the right image. ric / tic are the batch's extrinsics
 *              state; the call reads no field of vilo_config.
 * Outputs per landmark, concatenated window by window, inside a window in the caller's vilo_window_desc order (as vilo_batch_triangulate):
 *   pts_cam [sum L][3]        zeros for a landmark that is not predicted
 *   pts_cam_right [sum L][3]  (may be NULL) the same for the right camera
 *   flags [sum L]             (may be NULL) bit 0: predicted; bit 1: pts_cam.z is not positive (behind the next left camera: a projection
 *                             would divide by it); bit 2: a component of pts_cam (or pts_cam_right) is not finite; bit 3: as bit 1 for
 *                             pts_cam_right. 0 for a landmark that is not predicted.
 * Outputs per window: next_pose[w][7] (may be NULL) = [P_n, q_n] and records[w] (may be NULL): n_predicted, the number of landmarks with
 * bit 0 set, and status:
 *   VILO_PREDICT_OK
 *   VILO_PREDICT_TOO_FEW_FRAMES  constant-velocity mode with n_frames < 3 (the reference's `frame_count < 2` return, :1697). In
 *                                VILO_PREDICT_GIVEN a window of two frames predicts as any other.
 *   VILO_PREDICT_NUMERIC         a value that is not finite in the poses of the window's frames, in its extrinsics (the right camera's only
 *                                when pts_cam_right is given), in next_pose_in[w] or in the next pose formed (a zero quaternion).
 * For any status but OK nothing is predicted (pts_cam zeros, flags 0, n_predicted 0), next_pose[w] is frame k's current pose bit for bit, and
 * the other windows of the batch are not affected.
 * Side effects: none, and no option to have any: nothing of the state is being estimated. The call's device memory is returned when it
 * returns. Every output of a window is bitwise independent of the batch it shares and of its position in it. A batch whose windows have
 * no landmarks still reports next_pose and records; the landmark arrays are not touched. opts NULL: vilo_default_predict_opts.
 * Bad arguments (VILO_ERR_BAD_ARG, the caller's arrays untouched): NULL ctx or batch, NULL pts_cam with landmarks present, an unknown mode,
 * VILO_PREDICT_GIVEN without next_pose_in. */
#define VILO_PREDICT_CONSTANT_VELOCITY 0
#define VILO_PREDICT_GIVEN 1
#define VILO_PREDICT_OK 0
#define VILO_PREDICT_TOO_FEW_FRAMES 1
#define VILO_PREDICT_NUMERIC 2
typedef struct {
  int32_t mode;             /* VILO_PREDICT_CONSTANT_VELOCITY / VILO_PREDICT_GIVEN */
  int32_t pad;
} vilo_predict_opts;
void vilo_default_predict_opts(vilo_predict_opts *o);
typedef struct {
  int32_t n_predicted;
  int32_t status;           /* VILO_PREDICT_* */
} vilo_window_predict_record;

int vilo_batch_predict_next_frame(vilo_ctx *ctx, vilo_batch *batch, const vilo_predict_opts *opts, const double *next_pose_in, double *pts_cam,
                                  double *pts_cam_right, uint8_t *flags, double *next_pose, vilo_window_predict_record *records);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_predict_next_frame(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                   const vilo_predict_opts *opts, const double *next_pose_in, double *pts_cam, double *pts_cam_right,
                                   uint8_t *flags, double *next_pose, vilo_window_predict_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_predict_next_frame: k_predict_next_frame and k_predict_windows, without the
 * upload of next_pose_in and the copies out. */
double vilo_last_predict_ms(const vilo_ctx *ctx);

/* ---- mid-point dead reckoning of a frame's state through IMU samples (Estimator::processIMULeg, estimator.cpp:639-646, run on every
 * IMU / leg message on the newest frame, which starts as a copy of the frame before it, :794-802; fastPredictIMU / updateLatestStates,
 * :1800-1840, run the same recurrence again after every image) ----
 * State: the batch's current state, what vilo_batch_download returns. Per window, with f = opts->from_frame (-1: the window's last frame)
 * and the window's samples [offsets[w], offsets[w + 1]) in vilo_preintegrate's convention: the first sample of the range plays
 * (acc_0, gyr_0) and its dt is ignored (not even read), every later sample is one step. Only dt, acc and gyr of a sample are read.
 *   start  P, V, Ba, Bg of frame f; R = R(q_f / |q_f|); g = (0, 0, cfg.g_norm)
 *   step   with sample s after the previous sample s0 (:639-646, in this order of operations):
 *            un_acc_0 = R (s0.acc - Ba) - g
 *            un_gyr   = 1/2 (s0.gyr + s.gyr) - Bg
 *            R        = R * R(deltaQ(un_gyr s.dt))        deltaQ = (1, theta / 2) un-normalised (utility.h:28-41) and Eigen's
 *                                                         toRotationMatrix, which does not normalise either: the reference, literally
 *            un_acc_1 = R (s.acc - Ba) - g
 *            un_acc   = 1/2 (un_acc_0 + un_acc_1)
 *            P        = P + V dt + 1/2 dt^2 un_acc
 *            V        = V + dt un_acc
 *   state  [P(3), Quaterniond(R) as x y z w, V(3)]: what vector2double (:852-866) hands the solver for that frame. The quaternion is NOT
 *          re-normalised and R is not re-orthogonalised: R drifts from a rotation at second order in |un_gyr dt| per step, exactly as
 *          the reference's Rs[j] does between two images. vilo_batch_predict_next_frame normalises the pose it is given; the solver's
 *          PoseLocalParameterization normalises at its first step.
 * Outputs: state_out[w][10], the state after the window's last step; trajectory_out (may be NULL) [sum n_steps][10], the state after every
 * step, window by window in batch order (window w's rows start at the sum of the n_steps before it; its last row is state_out[w] bit
 * for bit); records[w] (may be NULL): n_steps = max(0, offsets[w + 1] - offsets[w] - 1), whatever the status, and status:
 *   VILO_DR_OK        a range of 0 or 1 samples makes no step; state_out then goes through the same path: P, Quaterniond(R(q_f / |q_f|)), V
 *   VILO_DR_NO_FRAME  the window has no frame f; with opts->write also: it has no frame f + 1
 *   VILO_DR_NUMERIC   a value that is not finite in the start state (P, q, V, Ba, Bg of frame f), in a sample value the range reads, or
 *                     in the result
 * For NO_FRAME and NUMERIC state_out[w] and the window's trajectory rows are zeros and nothing is written; the other windows of the batch
 * are not affected.
 * Side effects: with opts->write == 0 none. With opts->write == 1, for the windows with status OK, P, the quaternion and V become the
 * current pose and velocity of frame f + 1 (the reference's newest frame) and nothing else changes, not that frame's biases or leg
 * biases: vilo_batch_reset still restores the uploaded state; a following vilo_batch_solve (plain launches or the captured graph) starts
 * from the new state. write needs an explicit from_frame: the frame after a window's last does not exist.
 * The call's device memory is returned when it returns. Every output of a window is bitwise independent of the batch it shares and of
 * its position in it. opts NULL: vilo_default_dead_reckon_opts.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched, the caller's arrays untouched): NULL ctx or batch; with windows present NULL offsets
 * or state_out; offsets[0] != 0 or offsets decreasing; NULL samples with offsets[W] > 0; from_frame below -1 or above
 * VILO_MAX_FRAMES - 1; write other than 0 or 1; write == 1 with from_frame == -1. */
#define VILO_DR_OK 0
#define VILO_DR_NO_FRAME 1
#define VILO_DR_NUMERIC 2
typedef struct {
  int32_t from_frame;       /* -1: each window's last frame; else 0 .. VILO_MAX_FRAMES - 1 */
  int32_t write;            /* 1: the result becomes the current pose and velocity of frame from_frame + 1 (status OK only) */
} vilo_dead_reckon_opts;
void vilo_default_dead_reckon_opts(vilo_dead_reckon_opts *o);
typedef struct {
  int32_t n_steps;
  int32_t status;           /* VILO_DR_* */
} vilo_window_dead_reckon_record;

int vilo_batch_dead_reckon(vilo_ctx *ctx, vilo_batch *batch, const vilo_dead_reckon_opts *opts, const vilo_sample *samples,
                           const int32_t *offsets, double *state_out, double *trajectory_out, vilo_window_dead_reckon_record *records);
/* The same for host windows at the given states (SlidingWindow::processIMULeg, cerberus_amd/host/vilo_sliding_window.cpp, is the
 * one-robot host form): one batch is created and destroyed; with opts->write the new rows are written into state[w].pose and
 * state[w].speed_bias. */
int vilo_window_dead_reckon(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                            const vilo_dead_reckon_opts *opts, const vilo_sample *samples, const int32_t *offsets, double *state_out,
                            double *trajectory_out, vilo_window_dead_reckon_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_dead_reckon: k_dead_reckon, without the packing and upload of the samples
 * and the copies out. */
double vilo_last_dead_reckon_ms(const vilo_ctx *ctx);

/* ---- covariance of a frame's state carried through IMU samples (the error-state recurrence of IntegrationBase::midPointIntegration,
 * integration_base.h:103-137, written in the world frame beside vilo_batch_dead_reckon's nominal state) ----
 * The IMU-rate odometry vilo_batch_dead_reckon produces, with its uncertainty: per window, f = opts->from_frame (-1: the window's last
 * frame) and the samples [offsets[w], offsets[w + 1]) in vilo_batch_dead_reckon's convention (the first sample of the range plays
 * (acc_0, gyr_0), its dt is not read; every later sample is one step).
 *   nominal  P, R, V, Ba, Bg are vilo_batch_dead_reckon's: the same start, the same step in the same order of operations, the
 *            un-normalised R(deltaQ(.)). state_out[w][10] is bit for bit what vilo_batch_dead_reckon returns for the same arguments.
 *   error    15 coordinates, in the order and meaning of the leading 15 entries of vilo_batch_covariance's frame block: dp (world),
 *            dtheta (body frame, right perturbation), dv (world), dba, dbg: IntegrationBase's O_P, O_R, O_V, O_BA, O_BG.
 *   start    Sigma = cov_in[w] (15 x 15, row-major). Only the upper triangle with the diagonal is read; the lower is taken as its mirror.
 *            cov_in NULL: zero. (The leg bias does not enter the IMU recurrence: the leading 15 x 15 of a 19 x 19 frame block is the
 *            marginal to pass.)
 *   step     with sample s after s0, dt = s.dt, R0 the nominal R before the step's update and R1 after it:
 *              Sigma <- F Sigma F^T + V Q V^T
 *            F (15 x 15) and V (15 x 18) are the blocks of integration_base.h:103-132 with delta_q.toRotationMatrix() -> R0,
 *            result_delta_q.toRotationMatrix() -> R1, linearized_ba / bg -> the frame's Ba, Bg, and R_w_x, R_a_0_x, R_a_1_x the skew
 *            matrices of the nominal step's un_gyr, s0.acc - Ba, s.acc - Ba. With a = dt^2 / 4, h = dt / 2, A = R0 R_a_0_x,
 *            C = R1 R_a_1_x, K = I - R_w_x dt:
 *              F = [ I   -a (A + C K)   dt I   -a (R0 + R1)    a dt C ]      V = [ a R0   -a h C   a R1   -a h C   0      0    ]
 *                  [ 0    K             0       0             -dt I   ]          [ 0       h I     0       h I     0      0    ]
 *                  [ 0   -h (A + C K)   I      -h (R0 + R1)    h dt C ]          [ h R0   -h h C   h R1   -h h C   0      0    ]
 *                  [ 0    0             0       I              0      ]          [ 0       0       0       0       dt I   0    ]
 *                  [ 0    0             0       0              I      ]          [ 0       0       0       0       0      dt I ]
 *            Gravity does not appear: it is constant.
 *   Q        the 18 x 18 diagonal exactly as vilo_preintegrate_imu builds it (kernels_preint.hip, preint_imu_body, the line marked
 *            integration_base.h:31-37): cfg.acc_n^2 (3), gyr_n^2 (3), acc_n^2 (3), gyr_n^2 (3), acc_w^2 (3), gyr_w^2 (3). ACC_N on all
 *            three axes: cfg.acc_n_z belongs to the leg record and does not enter.
 * Outputs: cov_out[w][15][15], full, stored from the upper triangle so that it is bitwise symmetric; pose_cov_trajectory (may be NULL)
 * [sum n_steps][6][6], the pose block (dp, dtheta) after every step in vilo_batch_dead_reckon's trajectory order, what an odometry
 * message's covariance field holds (a window's last row is the pose block of cov_out[w] bit for bit); state_out[w][10]; records[w] (may
 * be NULL) = {n_steps, status}. A range of 0 or 1 samples makes no step: cov_out[w] is then the mirrored cov_in[w] (or zeros), bit for bit.
 * Statuses: VILO_DR_OK / VILO_DR_NO_FRAME / VILO_DR_NUMERIC with vilo_batch_dead_reckon's meaning; NUMERIC also for a value that is not
 * finite in the triangle of cov_in[w] that is read, or in the resulting covariance. For a failed window state_out[w], cov_out[w] and
 * its trajectory rows are zeros; the other windows of the batch are not affected.
 * Side effects: none; there is no write option (the call is no state-changing call). The call's device memory is returned when it
 * returns. Every output of a window is bitwise independent of the batch it shares and of its position in it. opts NULL:
 * vilo_default_dr_cov_opts.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched, the caller's arrays untouched): as for vilo_batch_dead_reckon, and with windows
 * present a NULL cov_out; reserved other than 0. */
typedef struct {
  int32_t from_frame;       /* -1: each window's last frame; else 0 .. VILO_MAX_FRAMES - 1 */
  int32_t reserved;         /* 0 */
} vilo_dr_cov_opts;
void vilo_default_dr_cov_opts(vilo_dr_cov_opts *o);

int vilo_batch_dead_reckon_covariance(vilo_ctx *ctx, vilo_batch *batch, const vilo_dr_cov_opts *opts, const vilo_sample *samples,
                                      const int32_t *offsets, const double *cov_in, double *state_out, double *cov_out,
                                      double *pose_cov_trajectory, vilo_window_dead_reckon_record *records);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_dead_reckon_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                       const vilo_dr_cov_opts *opts, const vilo_sample *samples, const int32_t *offsets, const double *cov_in,
                                       double *state_out, double *cov_out, double *pose_cov_trajectory,
                                       vilo_window_dead_reckon_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_dead_reckon_covariance: k_dr_covariance, without the packing and upload
 * of the samples and of cov_in and the copies out. */
double vilo_last_dr_cov_ms(const vilo_ctx *ctx);

/* ---- leg-odometry dead reckoning of a frame through samples (the nominal-state part of IMULegIntegrationBase::midPointIntegration,
 * imu_leg_integration_base.cpp:152-158 and :181-351, with propagate()'s carry, :121-135; literally and in that order of operations,
 * without the Jacobian, covariance, g / h and noise_diag work) ----
 * Where the body is according to the legs, the body velocity each leg reports, which feet the contact model counts as standing, the
 * weight each leg gets in the fused velocity and where the feet are in the world, at sensor rate. A batch of use_leg windows only.
 * State: the batch's current state. Per window, with f = opts->from_frame (-1: the window's last frame) and the window's samples
 * [offsets[w], offsets[w + 1]) in vilo_preintegrate's convention: the first sample of the range plays (acc_0, gyr_0, phi_0, dphi_0, c_0)
 * and its dt is not read; every later sample is one step.
 *   start  delta_q = identity, delta_v = 0, delta_eps[j] = 0, sum_delta_eps = 0, sum_dt = 0 (:7-47). The linearisation point is frame f's
 *          Ba, Bg and leg biases rho of the current state, with rho_fix, p_br, R_br of the context's config. The contact-force filter of
 *          contact_sensor_type 2 starts as a fresh object's (min, max, variance, window and index all zero), exactly as
 *          vilo_preintegrate starts it.
 *   step   with sample s after the previous sample s0, dt = s.dt:
 *            :152-158  un_acc_0 = delta_q (s0.acc - Ba); un_gyr = 1/2 (s0.gyr + s.gyr) - Bg;
 *                      result_delta_q = delta_q * (1, un_gyr dt / 2), un-normalised; un_acc_1 = result_delta_q (s.acc - Ba);
 *                      result_delta_v = delta_v + 1/2 (un_acc_0 + un_acc_1) dt. (delta_p, :157, reaches no output and is not carried.)
 *            :183-229  foot_contact_flag[j]: contact_sensor_type 0 and 1: s.c[j] >= 0.5. Type 2: force = 1/2 (s0.c[j] + s.c[j]) through the
 *                      min / max filter with its decays 0.9991 / 0.997, threshold = min + v_n_force_thres_ratio (max - min), the
 *                      logistic 1 / (1 + exp(-v_n_term1_steep (force - threshold))) TRUNCATED to 0 or 1 (foot_contact_flag is a
 *                      Vector4i), and the variance over the five-slot window the force has just entered (sum in slot order, / 4).
 *            :232-257  v = -R_br jac(phi) dphi - [gyr - Bg]x (p_br + R_br fk(phi)) of s0 and of s (A1Kinematics at rho[j], rho_fix[j]);
 *                      lo_v_j = 1/2 (delta_q v(s0) + result_delta_q v(s)); delta_eps[j] += lo_v_j dt.
 *            :290-317  uncertainties: types 0 / 1: (n_xy, n_xy, n_z), n = v_n_max (1 - flag) + flag v_n_min_xy (or _z). Type 2:
 *                      (v_n_max (1 - flag) + v_n_min + v_n_term2_var_rescale variance) + v_n_term3_distance_rescale (lo_v_j - delta_v)^2
 *                      per component, delta_v the one BEFORE the step.
 *            :333-351  w_j = (v_n_max + v_n_term2_var_rescale + v_n_term3_distance_rescale) / uncertainty, per component, at least
 *                      0.001; sum_delta_eps += (sum_j w_j o lo_v_j dt) / (sum_j w_j), component-wise, j = 0, 1, 2, 3 in that order.
 *                      The weights stay component-wise in frame f's body frame, as in the reference: nothing is rotated before weighting.
 *            :354-358  (all four flags 0) only overwrites uncertainties that go to noise_diag, after the weights were taken: it
 *                      changes nothing here.
 *            :121-135  delta_q = result_delta_q / |result_delta_q|, delta_v = result_delta_v, sum_dt += dt, s becomes s0.
 *   world  R0 = R(q_f / |q_f|), P0 = frame f's position. Fused leg position P0 + R0 sum_delta_eps; leg j's P0 + R0 delta_eps[j]: what the
 *          IMU-leg factor's epsilon rows compare with R_i^T (P_j - P_i).
 * delta_q, delta_v and delta_eps are those of vilo_preintegrate on the same samples at the same linearisation point, and through it of
 * the reference (pinned at 1e-12). sum_delta_eps, the weights and the flags have no public counterpart in the pinned oracle (the
 * reference's result_sum_delta_epsilon is not part of vilo_preint): they are restated from the lines above, unpinned.
 * Outputs:
 *   state_out[w][32]  after the last step: sum_dt [0], delta_q x y z w [1..5), delta_v [5..8), delta_eps [8..20), sum_delta_eps [20..23),
 *                     fused world position [23..26), the last step's foot_contact_flag [26..30) (zeros without a step), zeros [30..32).
 *   legs_out[w][12]   leg j's world position at [3 j .. 3 j + 3).
 *   trajectory_out    (may be NULL) [sum n_steps][48], one row per step, window by window in batch order as vilo_batch_dead_reckon's:
 *                     sum_dt [0], fused world position [1..4), fused world velocity of the step R0 (sum_j w_j o lo_v_j / sum_j w_j)
 *                     [4..7), foot_contact_flag [7..11), R0 lo_v_j [11 + 3 j ..), w_j [23 + 3 j ..), foot j in the world
 *                     fused position + R0 result_delta_q (p_br + R_br fk(s.phi)) [35 + 3 j ..), zero [47]. A window's last row agrees
 *                     bit for bit with its state_out (sum_dt, position, flags). The state_out of a call is bit for bit the same with
 *                     and without a trajectory.
 *   records[w]        (may be NULL) n_steps = max(0, offsets[w + 1] - offsets[w] - 1), whatever the status, and the status:
 *                     VILO_DR_OK; VILO_DR_NO_FRAME: the window has no frame f; VILO_DR_NUMERIC: a value that is not finite in the start
 *                     (P, q, Ba, Bg, rho of frame f), in a sample value the range reads (with at least one step: everything but the first
 *                     sample's dt), or in state_out / legs_out. For NO_FRAME and NUMERIC the window's rows of all three arrays are zeros;
 *                     the other windows are not affected.
 * Side effects: none, and there is no write option: current and uploaded state, records, mask, snapshot and summaries stay bytewise as
 * they were. The call's device memory is returned when it returns. Every output of a window is bitwise independent of the batch it
 * shares and of its position in it. opts NULL: vilo_default_leg_dead_reckon_opts. A batch of use_leg == 0 windows: VILO_ERR_UNSUPPORTED.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched, the caller's arrays untouched): as for vilo_batch_dead_reckon (NULL ctx or batch;
 * with windows present NULL offsets or state_out; offsets[0] != 0 or offsets decreasing; NULL samples with offsets[W] > 0; from_frame
 * below -1 or above VILO_MAX_FRAMES - 1), and with windows present NULL legs_out; reserved other than 0. */
typedef struct {
  int32_t from_frame;       /* -1: each window's last frame; else 0 .. VILO_MAX_FRAMES - 1 */
  int32_t reserved;         /* 0 */
} vilo_leg_dead_reckon_opts;
void vilo_default_leg_dead_reckon_opts(vilo_leg_dead_reckon_opts *o);
typedef struct {
  int32_t n_steps;
  int32_t status;           /* VILO_DR_* */
} vilo_window_leg_dead_reckon_record;

int vilo_batch_leg_dead_reckon(vilo_ctx *ctx, vilo_batch *batch, const vilo_leg_dead_reckon_opts *opts, const vilo_sample *samples,
                               const int32_t *offsets, double *state_out, double *legs_out, double *trajectory_out,
                               vilo_window_leg_dead_reckon_record *records);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_leg_dead_reckon(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                const vilo_leg_dead_reckon_opts *opts, const vilo_sample *samples, const int32_t *offsets,
                                double *state_out, double *legs_out, double *trajectory_out, vilo_window_leg_dead_reckon_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_leg_dead_reckon: k_leg_dead_reckon, without the packing and upload of the
 * samples and the copies out. */
double vilo_last_leg_dead_reckon_ms(const vilo_ctx *ctx);

/* ---- covariance of a frame's leg-odometry state carried through samples (the error-state recurrence of
 * IMULegIntegrationBase::midPointIntegration, imu_leg_integration_base.cpp:288-468, written in the world frame beside
 * vilo_batch_leg_dead_reckon's nominal state) ----
 * How uncertain the legs' answer is, at sensor rate: a foot in the air carries v_n_max, a standing foot v_n_min_*. A batch of use_leg
 * windows only. Arguments as vilo_batch_leg_dead_reckon: f = opts->from_frame (-1: the window's last frame) and the samples
 * [offsets[w], offsets[w + 1]) in vilo_preintegrate's convention (the first sample of the range plays the _0 values, its dt is not read;
 * every later sample is one step).
 *   nominal  exactly vilo_batch_leg_dead_reckon's (legdr_host.hpp's legdr_step, called): state_out[w][32] and legs_out[w][12] are bit for
 *            bit what that call returns for the same arguments.
 *   error    31 coordinates in the reference's ILStateOrder (parameters.h:135-149): dp (0), dtheta (3), dv (6), deps_1..4 (9 .. 20),
 *            dba (21), dbg (24), drho_1..4 (27 .. 30). dtheta is the body-frame right perturbation; dp, dv and deps_j are in the WORLD
 *            frame; deps_j is the error of leg j's world position P0 + R0 delta_eps[j], that is, of legs_out.
 *   start    cov_in[w][19][19] is the frame block of vilo_batch_covariance (dp dtheta dv dba dbg drho), row-major. Only the upper triangle
 *            with the diagonal is read; cov_in NULL: zero. Sigma_0 = E cov_in E^T with E (31 x 19): the frame block's rows go to
 *            P, R, V, BA, BG, RHO, and the dp rows also into each of the four eps_j row groups (a leg's world position starts at the
 *            frame's position and shares its error).
 *   step     with sample s after s0, dt = s.dt, R_f = R(q_f / |q_f|), R0 = R_f R(delta_q) before the step, R1 = R_f R(result_delta_q)
 *            (un-normalised, :154), Ba, Bg, rho the frame's:   Sigma <- F Sigma F^T + V Q V^T
 *            F (31 x 31) and V (31 x 46) are the blocks of :376-465 with delta_q.toRotationMatrix() -> R0,
 *            result_delta_q.toRotationMatrix() -> R1 and linearized_ba / bg / rho -> the frame's biases; every other operand is the
 *            nominal step's own value. With a = dt^2 / 4, h = dt / 2, A0 = [s0.acc - Ba]x, A1 = [s.acc - Ba]x, C = R1 A1,
 *            K = kappa_7 = I - [un_gyr]x dt, S = R0 + R1, and per leg j and endpoint e (0: s0, 1: s) v_e (:242-243),
 *            p_e = p_br + R_br fk(phi_e), J_e = jac(phi_e), g_e, h_e (:272-286 without their leading rotation, g without its sign):
 *              row      dtheta                          dv      deps_j   dba      dbg                                       drho_j
 *              dp       -a (R0 A0 + C K)                dt I             -a S      a dt C
 *              dtheta   K                                                         -dt I
 *              dv       -h (R0 A0 + C K)                I                -h S      h dt C
 *              deps_j   -h (R0 [v_0]x + R1 [v_1]x K)            I                  h dt R1 [v_1]x - h (R0 [p_0]x + R1 [p_1]x)   -h (R0 g_0 + R1 g_1)
 *              dba, dbg, drho_j: unit rows; dp and deps_j: unit columns
 *            V, by noise block (acc_0, gyr_0, acc_1, gyr_1, acc_w, gyr_w, phi_0, phi_1, dphi_0, dphi_1, v_1..4 (3 each), rho_1..4):
 *              dp       a R0 | -a h C | a R1 | -a h C
 *              dtheta        |  h I   |      |  h I
 *              dv       h R0 | -h h C | h R1 | -h h C
 *              deps_j        | -h h R1 [v_1]x + h R0 [p_0]x |  | -h h R1 [v_1]x + h R1 [p_1]x | phi: -h R0 h_0, -h R1 h_1 |
 *                            dphi: -h R0 R_br J_0, -h R1 R_br J_1 | v_j: -dt R_f
 *              dba: acc_w -dt I; dbg: gyr_w -dt I; drho_j: rho_j -dt
 *            Gravity does not appear: it is constant. The v_j block is -I dt in the reference (:456), with no rotation to substitute; the
 *            uncertainties it carries are per axis of frame f's body frame (n_xy is not n_z), so in the world frame it is -dt R_f:
 *            the (deps_j, deps_j) block receives dt^2 R_f diag(uncertainties_j) R_f^T. With -dt I the relation to the record below
 *            would fail by up to 4e-6 under contact models 0 and 1.
 *   Q        the 46-entry diagonal of :288-374, per step, from that step's foot_contact_flag and foot_force_var:
 *            (acc_n, acc_n, acc_n_z)^2 (acc_n_z DOES enter here), gyr_n^2 (3), those six again, acc_w^2 (3), gyr_w^2 (3), phi_n^2 (6),
 *            dphi_n^2 (6), the twelve uncertainties of the contact model in force (types 0 / 1 :290-299; type 2 :300-317 with delta_v
 *            before the step) and the four rho_uncertainty = rho_c_n flag + rho_nc_n; when all four flags are 0 (:354-358) every
 *            uncertainty is 10e10 and every rho_uncertainty rho_nc_n. The uncertainties and rho_uncertainty are NOT squared, as the
 *            reference does not square them.
 *   record   with T = blkdiag(R_f, I3, R_f, R_f x 4, I3, I3, I4): F = T F_rec T^T, so
 *              Sigma_out = T (Phi Sigma_0' Phi^T + Sigma_rec) T^T,   Sigma_0' = T^T Sigma_0 T,
 *            Phi and Sigma_rec the jacobian and covariance of vilo_preintegrate's (the reference's) record of the same samples at a
 *            linearisation point equal to the frame's biases.
 * Outputs: cov_out[w][31][31], full, stored from the upper triangle so that it is bitwise symmetric; pose_cov_trajectory (may be NULL)
 * [sum n_steps][6][6], the (dp, dtheta) block after every step; leg_cov_trajectory (may be NULL) [sum n_steps][4][3][3], the diagonal
 * block of each deps_j, that is, the covariance of each leg's world position after every step; both in vilo_batch_leg_dead_reckon's
 * trajectory order, a window's last rows bit for bit the blocks of cov_out[w]; state_out[w][32], legs_out[w][12]; records[w] (may be
 * NULL) = {n_steps, status}. A range of 0 or 1 samples makes no step: cov_out[w] is then Sigma_0 bit for bit.
 * Statuses: VILO_DR_OK / VILO_DR_NO_FRAME / VILO_DR_NUMERIC with vilo_batch_leg_dead_reckon's meaning; NUMERIC also for a value that is
 * not finite in the triangle of cov_in[w] that is read, or in the resulting covariance. For a failed window every row of it in every
 * output is zeros; the other windows of the batch are not affected.
 * Not in it: a covariance of the fused position sum_delta_eps (the reference has none), packed-triangle transfers, a write option,
 * samples held under vilo_batch_set_samples.
 * Side effects: none. The call's device memory is returned when it returns. Every output of a window is bitwise independent of the batch
 * it shares and of its position in it. opts NULL: vilo_default_leg_dr_cov_opts. A batch of use_leg == 0 windows: VILO_ERR_UNSUPPORTED.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched, the caller's arrays untouched): as for vilo_batch_leg_dead_reckon, and with windows
 * present a NULL cov_out; reserved other than 0. */
typedef struct {
  int32_t from_frame;       /* -1: each window's last frame; else 0 .. VILO_MAX_FRAMES - 1 */
  int32_t reserved;         /* 0 */
} vilo_leg_dr_cov_opts;
void vilo_default_leg_dr_cov_opts(vilo_leg_dr_cov_opts *o);

int vilo_batch_leg_dead_reckon_covariance(vilo_ctx *ctx, vilo_batch *batch, const vilo_leg_dr_cov_opts *opts, const vilo_sample *samples,
                                          const int32_t *offsets, const double *cov_in, double *state_out, double *legs_out,
                                          double *cov_out, double *pose_cov_trajectory, double *leg_cov_trajectory,
                                          vilo_window_leg_dead_reckon_record *records);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_leg_dead_reckon_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                           const vilo_leg_dr_cov_opts *opts, const vilo_sample *samples, const int32_t *offsets,
                                           const double *cov_in, double *state_out, double *legs_out, double *cov_out,
                                           double *pose_cov_trajectory, double *leg_cov_trajectory,
                                           vilo_window_leg_dead_reckon_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_leg_dead_reckon_covariance: k_leg_dr_covariance, without the packing and
 * upload of the samples and of cov_in and the copies out. */
double vilo_last_leg_dr_cov_ms(const vilo_ctx *ctx);

/* ---- double2vector's gauge fix on a resident batch (estimator.cpp:903-1003) ---------------------------------------------------------
 * After vilo_batch_solve the batch's device state is the raw solver output (para_*). The reference never reads that state:
 * Estimator::optimization() calls double2vector() right after ceres::Solve, and the marginalisation (:1247-1455), outliersRejection,
 * predictPtsInNextFrame, failureDetection (:1005-1052), slideWindow and updateLatestStates all read the re-anchored one. This call is that
 * step, in place on the batch's device state, so that every query of a batch (residuals, covariance, predict_next_frame, marginalize, ...)
 * can run where the reference runs it: solve -> gauge fix -> queries -> marginalisation.
 * Per window with F = n_frames, anchor pose (P_a, q_a) and solved frame-0 pose (P_0, q_0), literally :905-957:
 *   y_diff   = R2ypr(R(q_a)).x - R2ypr(R(q_0)).x                       (degrees; R2ypr as utility.h:87-99 writes it)
 *   rot      = ypr2R(y_diff, 0, 0); where | |pitch| - 90 | < 1 for either of the two R2ypr: rot = R(q_a) R(q_0)^T      (:925-934)
 *   frame i  : q_i <- Quaterniond(rot R(q_i / |q_i|)),  P_i <- rot (P_i - P_0) + P_a,  V_i <- rot V_i                  (i < F)
 *   camera c : q_c <- Quaterniond(R(q_c / |q_c|))  (:971-982: ric is a normalised quaternion's matrix; vector2double packs it back)
 * Biases, leg biases, td, the extrinsic translations and the inverse depths are not touched. It is the arithmetic of vilo_gauge_fix and
 * of vilo_optimize_windows (one device function, k_gauge_fix_body; the golden gauge_fix_edges.npz pins it at the Euler singularity).
 * anchor: VILO_GAUGE_ANCHOR_UPLOADED (default): frame 0's pose of the state the batch was created with (Rs[0], Ps[0] of before the solve;
 * vilo_optimize_windows uses the same). VILO_GAUGE_ANCHOR_GIVEN: anchor_pose [W][7] as [px py pz qx qy qz qw]: the reference's
 * failure_occur branch (:908-913: last_R0, last_P0), or a batch solved more than once without a reset, where the state before the second
 * solve is the caller's to name.
 * Outputs (each may be NULL): records[w] = {yaw_diff_deg (y_diff above), singular (1: the :925-934 branch was taken), status};
 * pose0_before [W][7]: the solver's frame-0 pose that was replaced (as read, whatever the status).
 *   VILO_GAUGE_OK
 *   VILO_GAUGE_NUMERIC  a value the window's fix reads is not finite (the anchor pose, a pose or velocity of a frame below F, an extrinsic
 *                       quaternion that would be rewritten): nothing of that window is written, yaw_diff_deg and singular read 0
 * Constant blocks: a window with ex_const set keeps its extrinsic rows bit for bit as uploaded (the solver never moves them; rewriting
 * them with their normalised form would move a constant block by an ulp per call). vilo_optimize_windows and vilo_gauge_fix rewrite
 * the extrinsic quaternions of every window, constant or not, as they always have: their results stay what they were. On windows whose
 * extrinsics are free the two paths agree bit for bit.
 * Side effects: the pose, velocity and extrinsic-quaternion entries of the current state, nothing else. vilo_batch_reset still restores
 * the upload; a following vilo_batch_solve (plain launches or the captured graph) starts from the fixed state. The call's device memory
 * is returned when it returns. Every output of a window is bitwise independent of the batch it shares and of its position in it.
 * opts NULL: vilo_default_gauge_opts.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched): NULL ctx or batch; an anchor other than the two; GIVEN without anchor_pose;
 * anchor_pose without GIVEN. */
#define VILO_GAUGE_ANCHOR_UPLOADED 0
#define VILO_GAUGE_ANCHOR_GIVEN 1
#define VILO_GAUGE_OK 0
#define VILO_GAUGE_NUMERIC 1
typedef struct {
  int32_t anchor;           /* VILO_GAUGE_ANCHOR_* */
  int32_t reserved;         /* 0 */
} vilo_gauge_opts;
void vilo_default_gauge_opts(vilo_gauge_opts *o);
typedef struct {
  double yaw_diff_deg;
  int32_t singular;
  int32_t status;           /* VILO_GAUGE_* */
} vilo_window_gauge_record;
int vilo_batch_gauge_fix(vilo_ctx *ctx, vilo_batch *batch, const vilo_gauge_opts *opts, const double *anchor_pose,
                         vilo_window_gauge_record *records, double *pose0_before);
/* The same for host windows at the given states, each with its own n_frames (vilo_gauge_fix takes one F for all): one batch is created
 * and destroyed, the fixed pose, speed_bias and ex_pose rows are written into state[w]. The uploaded anchor is then state[w]'s own frame 0
 * (the fix only normalises); a solver result is fixed with VILO_GAUGE_ANCHOR_GIVEN. */
int vilo_window_gauge_fix(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_gauge_opts *opts,
                          const double *anchor_pose, vilo_window_gauge_record *records, double *pose0_before);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_gauge_fix: k_gauge_fix_x, without the anchor's upload and the copies out. */
double vilo_last_gauge_fix_ms(const vilo_ctx *ctx);

/* ---- Estimator::failureDetection on a resident batch (estimator.cpp:1005-1052) -----------------------------------------------------
 * The reference's function returns false on its first line: nothing below that line runs there and nothing reboots. This call evaluates
 * every criterion of the text below it, literally, as a flag bit per window, at the batch's device state, with n = n_frames - 1:
 *   bit 0  last_track_num < 2                                                  (:1008; caller's last_track_num [W], NULL: bit stays 0)
 *   bit 1  |Ba_n| > 2.5                                                        (:1013)
 *   bit 2  |Bg_n| > 1.0                                                        (:1018)
 *   bit 3  |P_n - last_P| > 5                                                  (:1031; caller's last_pose)
 *   bit 4  |P_n.z - last_P.z| > 1                                              (:1036; caller's last_pose)
 *   bit 5  acos(Quaterniond(R_n^T last_R).w()) * 2.0 / 3.14 * 180.0 > 50       (:1041-1046; caller's last_pose)
 * The batch holds only landmarks with used_num >= 4, so it cannot know the feature manager's last_track_num: the caller gives it.
 * last_pose [W][7] as [px py pz qx qy qz qw] is last_P, last_R of :840-841; NULL leaves bits 3 to 5 at 0. R_n = R(q_n / |q_n|) and
 * last_R = R(q_last / |q_last|). Bit 5 uses the reference's 3.14, not pi, and Eigen's matrix-to-quaternion conversion; an acos argument
 * above 1 by rounding gives NaN, and the comparison is then false, as in the reference.
 * records[w] = {flags, would_reboot, status}: would_reboot = bit 1 or bit 2, the only criteria whose branch says `return true` in the
 * text (the others' are commented out). values_out (may be NULL) [W][6]: the six compared quantities in bit order (last_track_num as a
 * double; 0 for those whose input array is NULL).
 *   VILO_FAILURE_OK
 *   VILO_FAILURE_NUMERIC  a value read is not finite (Ba_n, Bg_n; with last_pose also frame n's pose and last_pose[w]): flags,
 *                         would_reboot and the values read 0
 * No side effects. One launch, one code path for every batch size; every output of a window is bitwise independent of the batch it
 * shares and of its position in it.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched): NULL ctx or batch; with windows present NULL records. */
#define VILO_FAILURE_OK 0
#define VILO_FAILURE_NUMERIC 1
#define VILO_FAILURE_FEW_TRACKS 1
#define VILO_FAILURE_BIG_BA 2
#define VILO_FAILURE_BIG_BG 4
#define VILO_FAILURE_BIG_TRANSLATION 8
#define VILO_FAILURE_BIG_Z 16
#define VILO_FAILURE_BIG_ANGLE 32
typedef struct {
  int32_t flags;            /* VILO_FAILURE_* bits */
  int32_t would_reboot;     /* bit 1 or bit 2 */
  int32_t status;           /* VILO_FAILURE_OK / VILO_FAILURE_NUMERIC */
} vilo_window_failure_record;
int vilo_batch_failure_detection(vilo_ctx *ctx, vilo_batch *batch, const int32_t *last_track_num, const double *last_pose,
                                 vilo_window_failure_record *records, double *values_out);
/* The same for host windows at the given states: one batch is created and destroyed. */
int vilo_window_failure_detection(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                  const int32_t *last_track_num, const double *last_pose, vilo_window_failure_record *records,
                                  double *values_out);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_failure_detection: k_failure_detection alone. */
double vilo_last_failure_detection_ms(const vilo_ctx *ctx);

/* ---- re-propagate a resident batch's preintegration records once, at chosen biases (IMULegIntegrationBase::repropagate,
 * imu_leg_integration_base.cpp:62-86, IntegrationBase::repropagate, integration_base.h; the start-up loop of processImage,
 * estimator.cpp:752-760, and solveGyroscopeBias' trailing loop, initial_aligment.cpp:42-47) ----
 * The records are integrated again from their samples ONCE and the solves that follow run on fixed records, as the reference's do;
 * vilo_batch_set_samples instead integrates inside every iteration. Interval k of window w is f = 10 w + k; samples / offsets as for
 * vilo_batch_set_samples ([n_windows * 10 + 1] offsets, the first sample of a range the constructor's, empty ranges for intervals a
 * window does not have).
 * The point of interval k (opts->point):
 *   VILO_REPROP_POINT_STATE    (Ba_k, Bg_k, rho_k) of the batch's current state: the point the IMU factors correct towards and that
 *                              repropagate(Bai, Bgi, rhoi) under vilo_batch_set_samples uses
 *   VILO_REPROP_POINT_STARTUP  (0, Bg_{k+1}, rho_{k+1}): the reference's start-up loop, literally (interval k is
 *                              il_pre_integrations[k + 1], re-propagated at Vector3d::Zero(), Bgs[k + 1], Rhos[k + 1]); use_leg == 0:
 *                              IntegrationBase at (0, Bg_{k+1})
 *   VILO_REPROP_POINT_GIVEN    the caller's lin [n_windows * 10][10] = ba bg rho (use_leg == 0: the first 6 of a row are read)
 * Drift of interval k, of the record AS IT WAS: drift_ba = |point_ba - lin_ba|, drift_bg = |point_bg - lin_bg|, drift_rho =
 * |point_rho - lin_rho| (0 when use_leg == 0), 2-norms as sqrt(((d0 d0 + d1 d1) + d2 d2) [+ d3 d3]), every operation rounded.
 * Which intervals (opts->select):
 *   VILO_REPROP_SELECT_ALL      every interval of every window
 *   VILO_REPROP_SELECT_DRIFTED  those with NOT (drift_ba <= ba_threshold AND drift_bg <= bg_threshold AND drift_rho <= rho_threshold):
 *                               a drift above its threshold, or one that is not a number (a record whose own point is not finite)
 *   VILO_REPROP_SELECT_MASK     those with mask[f] != 0 (mask [n_windows * 10])
 * The thresholds are compared with the drifts above, in the units of the biases (m/s^2, rad/s, m); they are the caller's to set. The
 * defaults (0.10 / 0.01 / 0.01) are a starting point only: the reference has no such test, it re-propagates every interval at start-up
 * and none afterwards.
 * records[f] (may be NULL) = {drift_ba, drift_bg, drift_rho, selected, status}:
 *   VILO_REPROP_OK            selected; with write == 1 the record was replaced
 *   VILO_REPROP_NOT_SELECTED  the selection left it out (selected 0)
 *   VILO_REPROP_NO_INTERVAL   k >= n_frames - 1 (selected 0, drifts 0)
 *   VILO_REPROP_NO_SAMPLES    selected, write == 1 and the interval has fewer than two samples: the record is untouched
 *   VILO_REPROP_NUMERIC       the point is not finite: the record is untouched, selected 0, drifts 0
 * opts->write == 0 is the drift query: samples and offsets may be NULL, nothing is integrated, the batch is left bitwise as it was, and
 * drift_*, selected and status (OK / NOT_SELECTED / NO_INTERVAL / NUMERIC) come back.
 * opts->write == 1: for a selected interval with status OK the record becomes, bit for bit, what vilo_preintegrate (use_leg == 0:
 * vilo_preintegrate_imu) returns for the same samples at the same point, and its prepared form the sqrt_info vilo_batch_prepare
 * computes of it (under the vilo_set_sqrt_info_mode in force at this call). That is a fresh IMULegIntegrationBase object. For
 * contact_sensor_type 0 and 1 it is also what the reference's repropagate() gives. For type 2 the reference's repropagate() keeps the
 * contact-force filter the previous pass over the samples left in the object (imu_leg_integration_base.cpp:62-86 resets everything but
 * foot_force_min / max / window / var); this call does NOT: a batch holds no object state between calls, and a result that depended on
 * how often a record had been integrated before would not be reproducible. Intervals with sum_dt > 10 s, which carry no factor, are
 * re-propagated like any other (the reference loops over all of them). Every output of an interval, the record included, is bitwise
 * independent of the batch it shares and of its position in it.
 * Side effects with write == 1: the selected OK records and their prepared form are overwritten, nothing else of the records; win_bad
 * (the windows a covariance without sqrt_info fails) is rebuilt from the flags of the preparations in force, as
 * vilo_batch_set_samples(NULL) rebuilds it. States, landmarks, observations and the prior are not touched; vilo_batch_reset still restores
 * the states only. The device buffers keep their addresses: a captured solve graph stays valid and the next vilo_batch_solve may replay
 * it. A batch whose records went up in the compact form (only what the factors read) holds full records where this call wrote them:
 * both triangles of the covariance, every Jacobian entry. The call's device memory is returned when it returns.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing launched): NULL ctx or batch; an unknown point or select; write other than 0 or 1; GIVEN
 * without lin; MASK without mask; write == 1 without samples and offsets; offsets that decrease or are negative; a negative or
 * non-finite threshold. VILO_ERR_UNSUPPORTED: a batch without records on the device; records gathered from a vilo_preint_streams pool
 * (the pool's objects own them: reset and push there); vilo_batch_set_samples in force (the solve integrates every interval again at
 * every point anyway: switch it off first). A batch without windows: VILO_OK. opts NULL: vilo_default_reprop_opts. */
#define VILO_REPROP_POINT_STATE 0
#define VILO_REPROP_POINT_STARTUP 1
#define VILO_REPROP_POINT_GIVEN 2
#define VILO_REPROP_SELECT_ALL 0
#define VILO_REPROP_SELECT_DRIFTED 1
#define VILO_REPROP_SELECT_MASK 2
#define VILO_REPROP_OK 0
#define VILO_REPROP_NOT_SELECTED 1
#define VILO_REPROP_NO_INTERVAL 2
#define VILO_REPROP_NO_SAMPLES 3
#define VILO_REPROP_NUMERIC 4
typedef struct {
  int32_t point;            /* VILO_REPROP_POINT_* */
  int32_t select;           /* VILO_REPROP_SELECT_* */
  int32_t write;            /* 0: drift query, 1: integrate the selected intervals again */
  int32_t pad;
  double ba_threshold, bg_threshold, rho_threshold;   /* SELECT_DRIFTED: compared with drift_ba / drift_bg / drift_rho */
} vilo_reprop_opts;
void vilo_default_reprop_opts(vilo_reprop_opts *o);   /* STATE, ALL, write 1, thresholds 0.10 / 0.01 / 0.01 */
typedef struct {
  double drift_ba, drift_bg, drift_rho;
  int32_t selected;
  int32_t status;           /* VILO_REPROP_* */
} vilo_interval_reprop_record;
int vilo_batch_repropagate(vilo_ctx *ctx, vilo_batch *batch, const vilo_sample *samples, const int32_t *offsets, const vilo_reprop_opts *opts,
                           const double *lin, const uint8_t *mask, vilo_interval_reprop_record *records);
/* The same for host windows at the given states: one batch is created and destroyed; with opts->write the windows' preint (use_leg == 0:
 * preint_imu) arrays, which the descs point at, receive the selected OK records; the others are left as they are. */
int vilo_window_repropagate(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_sample *samples,
                            const int32_t *offsets, const vilo_reprop_opts *opts, const double *lin, const uint8_t *mask,
                            vilo_interval_reprop_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_repropagate: k_reprop_point and, with write, the integration,
 * k_reprop_commit, the preparation and the fold of win_bad, without the copies in and out. */
double vilo_last_repropagate_ms(const vilo_ctx *ctx);

/* ---- caller-given local steps on a resident batch's state (PoseLocalParameterization::Plus, pose_local_parameterization.cpp:12-27, on the
 *      7-dimensional blocks; Ceres' Plus of a Euclidean block, x + delta, on the others; Estimator::vector2double, estimator.cpp:848-901,
 *      for the host states a batch takes) ----
 * vilo_batch_retract computes x <- x [+] alpha * delta in place on the device state of every window, in the local coordinates
 * vilo_batch_gradient reports g and h in: what a line search, a gradient or preconditioned step of the caller's own, a teacher-forced
 * trajectory or a Monte-Carlo restart needs, without a new batch.
 * Inputs. state_step [W][222], or NULL for a zero step: exactly vilo_batch_gradient's state_grad layout (pose 11 x 6 (dp dtheta),
 * speed-bias 11 x 9, leg bias 11 x 4, extrinsics 2 x 6, td). lm_step [sum L], or NULL: the inverse depths' steps, window w's landmarks
 * concatenated window by window, inside a window in the caller's vilo_window_desc order (as every per-landmark array of this header).
 * alpha [W], or NULL for 1. opts->base: VILO_RETRACT_BASE_CURRENT (default) steps the current state; VILO_RETRACT_BASE_UPLOADED steps the
 * state the batch was created with, bit for bit what vilo_batch_reset followed by the call with CURRENT gives, in the same launch.
 * Arithmetic, fixed so that a host restatement agrees to the bit: s = alpha * delta, rounded once; a Euclidean coordinate becomes x + s,
 * rounded once (no fused multiply-add across the two); a pose or extrinsic block becomes vilo_pose_plus(x, s) — p + dp, q * deltaQ(dtheta)
 * normalised — through the device function vilo_pose_plus runs, so bit for bit its result.
 * Not stepped, whatever the step holds there (it is not read: NaN is harmless): the constant blocks (leg_bias_const, ex_const, td_const; the
 * leg biases of a use_leg == 0 window), the rows of frames a window does not have (n_frames < 11) and masked landmarks
 * (vilo_batch_mask_landmarks). Their bytes stay (with UPLOADED: become the uploaded ones, as after vilo_batch_reset).
 * Non-finite entries: a window with a non-finite alpha, or whose s is not finite in a coordinate that would be stepped, is not stepped at
 * all (the check comes before the window's first store; with UPLOADED it is reset) and reports VILO_RETRACT_NUMERIC; the other windows are
 * unaffected.
 * records [W] (optional): status; n_applied, the coordinates stepped (vilo_batch_gradient's n_free, less the masked landmarks); step_norm =
 * sqrt(sum s^2) and step_max = max |s| over them. A NUMERIC window reads 0 in all three.
 * What the call leaves alone: the uploaded copy (vilo_batch_reset and VILO_GAUGE_ANCHOR_UPLOADED still mean the state given at creation),
 * the preintegration records, the landmark mask, the solve summaries vilo_batch_download reports. A vilo_batch_solve after it starts from
 * the stepped state and may replay the captured launch sequence. One launch, one code path for every batch size; a window's state and
 * record are bitwise independent of the batch it shares and of its position in it. The call's device memory is returned when it returns.
 * Bad arguments (VILO_ERR_BAD_ARG, nothing written): NULL ctx or batch; a base other than the two; a reserved field that is not 0. */
#define VILO_RETRACT_BASE_CURRENT 0
#define VILO_RETRACT_BASE_UPLOADED 1
#define VILO_RETRACT_OK 0
#define VILO_RETRACT_NUMERIC 1
typedef struct {
  int32_t base;             /* VILO_RETRACT_BASE_* */
  int32_t reserved;         /* 0 */
} vilo_retract_opts;
void vilo_default_retract_opts(vilo_retract_opts *o);
typedef struct {
  int32_t status;           /* VILO_RETRACT_* */
  int32_t n_applied;        /* local coordinates stepped, inverse depths included */
  double step_norm;         /* sqrt(sum s_i^2) over them */
  double step_max;          /* max |s_i| over them */
} vilo_window_retract_record;
/* opts NULL: vilo_default_retract_opts (CURRENT). */
int vilo_batch_retract(vilo_ctx *ctx, vilo_batch *batch, const vilo_retract_opts *opts, const double *state_step, const double *lm_step,
                       const double *alpha, vilo_window_retract_record *records);
/* The same for host windows at the given states: one batch is created and destroyed, the stepped state is written into state[w] (the
 * uploaded state is then state[w] itself: the two bases agree). */
int vilo_window_retract(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_retract_opts *opts,
                        const double *state_step, const double *lm_step, const double *alpha, vilo_window_retract_record *records);
/* GPU time (HIP events on ctx's stream) of the last vilo_batch_retract: k_retract alone, without the copies in and out. */
double vilo_last_retract_ms(const vilo_ctx *ctx);

/* vector2double (estimator.cpp:848-901) for chosen windows of a resident batch: the host states state[i] replace the current device state
 * of window window_ids[i], i < n, as vilo_batch_create packs them (the inverse depths scattered through the batch's landmark order; rows
 * beyond a window's n_frames are not read). Windows that are not named stay bytewise as they were; the uploaded copy, the records, the mask
 * and the summaries are not touched. Bad arguments (VILO_ERR_BAD_ARG, nothing written): NULL ctx, batch, window_ids or state, n < 1, an id
 * outside 0 .. W - 1, an id named twice. */
int vilo_batch_set_state(vilo_ctx *ctx, vilo_batch *batch, int n, const int32_t *window_ids, const vilo_window_state *state);
/* GPU time of the last vilo_batch_set_state: k_set_state alone, without the upload. */
double vilo_last_set_state_ms(const vilo_ctx *ctx);

/* One snapshot slot per batch, for trial steps: save copies the current state (every window's 240 doubles and every inverse depth, masked
 * ones like any other) into the slot on the device, restore copies it back, bit for bit. The slot is allocated at the first save (2 KB per
 * window plus 8 B per landmark; a batch that never saves holds nothing more) and overwritten by every later one. State only: records, mask
 * and summaries are neither saved nor restored. vilo_batch_restore_state before any save returns VILO_ERR_UNSUPPORTED with vilo_last_error
 * saying so. Restore replaces the whole current state: a window named in a vilo_batch_set_state since the save comes back as saved like
 * any other. Both are asynchronous on the context's stream, as vilo_batch_reset is. */
int vilo_batch_save_state(vilo_ctx *ctx, vilo_batch *batch);
int vilo_batch_restore_state(vilo_ctx *ctx, vilo_batch *batch);

/* ---- measurement / test hooks (no counterpart in the reference) -------------------------------------- */
/* Windows of the last vilo_marginalize whose Amm was not certified positive definite beyond eps = 1e-8 and therefore went
 * through the eigen-thresholded pseudo-inverse of the full Amm (marginalization_factor.cpp:281-286) instead of block
 * elimination. The environment variable VILO_MARG_GENERAL=1 forces every window down that path. */
int vilo_debug_marg_general_count(const vilo_ctx *ctx);
/* Per-kernel GPU time of the solve pipeline, HIP events on ctx's stream. kinds: see vilo_kernel_name(). */
/* How sqrt_info = LLT(covariance.inverse()).matrixL().transpose() (imu_leg_factor.cpp:197-198, imu_factor.h) is computed for the batches and
 * factor evaluations that follow. 0 (default): Cholesky of the index-reversed covariance and a triangular inverse — the same matrix without
 * forming the inverse. 1: the reference's route literally (inverse by pivoted Gauss-Jordan elimination, then LLT). Both give the exact
 * matrix to a few 1e-15 row by row (the covariance's condition number of 1e13..1e14 is units: ~15 after diagonal equilibration), and the
 * whitened residuals / Jacobians of either agree with the compiled reference's to 1e-13 (tests/test_golden.py); mode 1 exists so that the
 * reference's formula is also there as written. */
int vilo_set_sqrt_info_mode(vilo_ctx *ctx, int mode);
/* Form of the prior's square root that vilo_marginalize / vilo_batch_marginalize / vilo_optimize_windows* leave (per context).
 * VILO_PRIOR_EIGEN (default): J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b over the eigenpairs with S > 1e-8, what MarginalizationInfo::marginalize
 * writes (marginalization_factor.cpp:297-305; rows of J0 mutually orthogonal, defined up to order and sign).
 * VILO_PRIOR_FACTOR: J0 = X^T, r0 = X_p^-1 b_p for the diagonally pivoted Cholesky factor X X^T = A' (n x r; a semi-definite A' — the
 * gauge directions — gives r < n, the rest of J0 is zero rows like the eigen form's dropped ones; X_p: its pivot rows), wherever the
 * device certifies that X X^T has no eigenvalue in (0, 1e-8]  (1 / |X_p^-1|_F^2 > 1e-8) — an orthogonal transformation of the eigen
 * form: J0^T J0, J0^T r0 and |r0|^2, which is all MarginalizationFactor::Evaluate's contribution to a solve depends on, are the same to
 * rounding, but the ROWS of J0 (and the residual vector of the factor) are in another basis. A window that cannot be certified gets the
 * eigen form. For callers that never look at J0 itself (a replay, a resident prior pool): a single window's marginalisation takes a
 * quarter of the time. */
#define VILO_PRIOR_EIGEN 0
#define VILO_PRIOR_FACTOR 1
int vilo_set_prior_form(vilo_ctx *ctx, int form);
/* Solver form of the batches this context solves from here on. VILO_SOLVER_AUTO (default) picks by batch size: eight waves per window
 * (one workgroup per window, its waves in fixed roles) up to 512 windows (VILO_MW8_MAX_WINDOWS; one per CU, a second round from 257 on), one wave up to 1024, the single wave in three kernels beyond. All
 * forms restate the same algorithm; the eight-wave form eliminates in another order and agrees with the single wave to rounding (1e-9 on
 * well-conditioned windows), SPLIT and WAVE agree bitwise. Pin a form when a window must get the same answer whatever the size of the
 * batch it shares. The environment variable VILO_SOLVER (wave | mw8 | split) only sets the default a context is created with. */
#define VILO_SOLVER_AUTO (-1)
#define VILO_SOLVER_WAVE 0
#define VILO_SOLVER_SPLIT 3
#define VILO_SOLVER_MW8 4
int vilo_set_solver_form(vilo_ctx *ctx, int form);
int vilo_get_solver_form(const vilo_ctx *ctx);
/* Batches created from here on may (1, default) or may not (0) use the compact 16-column visual rows / Gram slots (they apply while td
 * is a constant block in every window of the batch); the two row forms agree to rounding. VILO_NO_COMPACT=1 sets the default to 0. */
int vilo_set_compact_rows(vilo_ctx *ctx, int on);
/* Per-kernel HIP-event timing of the solve loop on the context's stream: 0 off (resident batches replay a hipGraph), 1 every kernel,
 * 2 + k only kernel kind k (vilo_kernel_name(k)). Resets the accumulated times. */
void vilo_set_profiling(vilo_ctx *ctx, int on);
int vilo_get_kernel_times(const vilo_ctx *ctx, double *ms, long long *launches, int n);
/* Test hook: DoglegStrategy's mu at the start of the following solves (default 1e-8 = Ceres' min_mu), to resume a solve from a state
 * (x, radius, mu) reached elsewhere: single steps are compared with the oracle this way (tests/test_branches.py). */
int vilo_debug_set_initial_mu(vilo_ctx *ctx, double mu);
const char *vilo_kernel_name(int kind);
/* Which form of each step the last vilo_batch_solve of `batch` ran: the launch sequence depends on the batch size, the number of packed
 * waves, the row form and the tuning switches read once per process (README "Environment switches"). Host bookkeeping only; a replay of
 * the captured sequence reports the forms it was captured with. out[8]:
 *   [0] visual linearisation: 0 k_lin_small_c (frame-parallel, IMU fused), 1 k_visual_linearize_tpar_c + k_visual_reduce,
 *       2 k_visual_linearize_tpar + k_visual_reduce (23 columns), 3 k_visual_linearize_pc_imu, 4 k_visual_linearize_pc,
 *       5 k_visual_linearize_c, 6 k_visual_linearize (23 columns); -1 none (no landmark in the batch, or no iteration)
 *   [1] IMU factors: 0 fused into the visual launch, 1 k_imu_raw + k_imu_linearize with one factor per wave, 2 the same with a pair per wave
 *   [2] fused IMU workgroups: 1 launched before the visual ones, 0 after them; -1 not fused
 *   [3] bookkeeping + assembly: 0 k_assemble_s, 1 the two-kernel compact assembly, 2 k_accept + k_assemble (23 columns)
 *   [4] solver: VILO_SOLVER_MW8, VILO_SOLVER_WAVE or VILO_SOLVER_SPLIT
 *   [5] visual rows: 1 compact (16 columns), 0 23 columns
 *   [6] 1: a replay of the captured launch sequence (hipGraph), 0: plain launches
 *   [7] launch order of the packed waves (VILO_WAVE_ORDER): 0 window order, 1 by length, 2 by length with groups rotated
 * Steps a solve did not launch read -1. VILO_ERR_BAD_ARG before the batch's first solve. */
int vilo_debug_batch_path(const vilo_batch *batch, int32_t out[8]);
/* Device memory of a batch: out[0] the bytes of the arena chunks it holds, out[1] the bytes handed out of them. A call on the batch gives
 * back what it took for itself: out[1] is the same before and after it (vilo_batch_residuals' first call adds its observation-row table). */
int vilo_debug_batch_device_bytes(const vilo_batch *batch, size_t out[2]);
/* Copy an internal device array of one window to the host (tests localise parity failures with it). */
int vilo_debug_fetch(vilo_ctx *ctx, vilo_batch *batch, int what, int win, double *out, int max_n);
/* Streams n doubles (8 B per lane) `reps` times: known byte count to calibrate rocprofv3 FETCH_SIZE / WRITE_SIZE. */
int vilo_debug_calib_copy(vilo_ctx *ctx, size_t n_doubles, int reps);

#ifdef __cplusplus
}
#endif
#endif /* VILO_GPU_H */
