// The cost of a window at a state, in pieces: the expressions inside the loops of the solver's cost kernels (k_visual_cost_walk, k_imu_cost,
// accept_body), of the residual call (kernels_resid.hip) and of the trial-cost call (kernels_trial.hip). A change of the observation rows,
// the td compensation, the Huber form, the IMU whitening or the prior's normal-equation form is made here and nowhere else. The pieces
// hold no state and take plain pointers and values (a kernel whose state is in LDS hands them LDS pointers and still reads with LDS
// loads); loops, barriers, LDS maps, outputs, the factor 1/2 and the order of the sums stay in the kernels, whose results are not bitwise
// equal to each other: the compiler contracts multiplies and adds differently in each.
//   OBS_*, obs_at                             rows of an observation by name; row r of frame t for a lane     every walk of the image
//   start_point                               td-compensated start-frame point in the body frame (p_i)       walk, residuals, trial cost
//   world_point, frame_point, camera_point    p_i -> world -> body frame j -> camera                         walk, residuals, trial cost
//   camera_block                              whitened residual pair, |r|^2, rho[0] of a camera block        walk, residuals, trial cost
//   imu_factor_raw, imu_stage                 raw residual of a factor; into the [entry][factor] LDS tile    k_imu_cost, k_resid_imu, k_trial_imu
//   imu_info_row, imu_row_dot                 masked row of sqrt_info; its product with a staged residual    the same three
//   prior_dx_block                            the prior's dx of one block, by its owner thread               those, marginalisation, gn_system.hpp
//   prior_row_term                            a row's part of dx^T (H dx + 2 b0)                             accept_body, residuals, trial cost
#pragma once
#include "batch_state.hpp"
#include "factors.hpp"
#include "solve_common.hpp"
#include "vilo_math.hpp"

// Rows of an observation (vilo_window_desc::obs, FeaturePerFrame: point, pointRight, velocity, velocityRight, cur_td). A packed wave's
// image is [t][OBS_ROWS][n_lanes] (batch_pack.hpp), t = 0 the landmark's start frame; obs_at: row r of frame offset t for a lane.
enum { OBS_LX = 0, OBS_LY, OBS_LZ, OBS_RX, OBS_RY, OBS_RZ, OBS_LVX, OBS_LVY, OBS_RVX, OBS_RVY, OBS_TD, OBS_ROWS };
__device__ __forceinline__ double obs_at(const double *obs, int n, int lane, int t, int r) { return (obs + (size_t)t * OBS_ROWS * n + lane)[(size_t)r * n]; }

// ---- visual part (the three Projection*Factor residuals) ----
// start-frame point in the body frame: (u0 u1 u2) the left point, (v0 v1) its velocity and t0 the td of the start row; inv_lam = 1 / lambda
__device__ __forceinline__ vilo::v3 start_point(double u0, double u1, double u2, double v0, double v1, double t0, double td, double inv_lam,
                                                const vilo::quat &qic, const vilo::v3 &tic) {
  const double dti = td - t0;
  return vilo::qrot(qic, vilo::mk3((u0 - v0 * dti) * inv_lam, (u1 - v1 * dti) * inv_lam, u2 * inv_lam)) + tic;
}
// body point of frame `pose` -> world, world -> body point of frame `pose`, body -> camera (qic, tic)
__device__ __forceinline__ vilo::v3 world_point(const double *pose, const vilo::v3 &p) { return vilo::qrot(vilo::ldq_pose(pose), p) + vilo::ld3(pose); }
__device__ __forceinline__ vilo::v3 frame_point(const double *pose, const vilo::v3 &p_w) { return vilo::qrot(vilo::qinv(vilo::ldq_pose(pose)), p_w - vilo::ld3(pose)); }
__device__ __forceinline__ vilo::v3 camera_point(const vilo::quat &qic, const vilo::v3 &tic, const vilo::v3 &p) { return vilo::qrot(vilo::qinv(qic), p - tic); }
// one camera block: r = sq (pcj.xy / pcj.z - (px py)), (px py) the td-compensated observation
struct CamBlock { double r0, r1, s2, rho0; };   // whitened residual pair, |r|^2, Huber's rho[0]
__device__ __forceinline__ CamBlock camera_block(const vilo::v3 &pcj, double px, double py, double sq, double huber_a) {
  CamBlock cb;
  const double inv_z = 1.0 / pcj.z;
  cb.r0 = sq * (pcj.x * inv_z - px);
  cb.r1 = sq * (pcj.y * inv_z - py);
  cb.s2 = cb.r0 * cb.r0 + cb.r1 * cb.r1;
  double rho[3];
  vilo::huber_rho(huber_a, cb.s2, rho);
  cb.rho0 = rho[0];
  return cb;
}

// ---- IMU part (IMULegFactor / IMUFactor, residuals only) ----
// the raw residual of factor f (interval f % 10 of its window) at the window's state x; leg: the window's use_leg. Rows 15..30 of the plain
// factor are zero, like every row of a factor that is not evaluated (ImuResid r = {}). The factors fill an array of this function's own:
// through the caller's (the returned object is one) the compiler merges their common tail into one store at a selected address before
// it sees the array, which then lands in scratch.
struct ImuResid { double r[31]; };
__device__ __forceinline__ ImuResid imu_factor_raw(const BatchDev &b, int f, const double *x, double g_norm, bool leg) {
  double t[31] = {};
  const PreintPrepared &pp = b.prep[f];
  const int k = f % 10;
  const double *pose = x + XO_POSE + 7 * k, *sb = x + XO_SB + 9 * k, *lb = x + XO_LB + 4 * k;
  if (leg) vilo::imu_leg_raw(pp.head, g_norm, pose, sb, lb, pose + 7, sb + 9, lb + 4, t, false, nullptr, 0);
  else vilo::imu_raw(pp.head, g_norm, pose, sb, pose + 7, sb + 9, t, false, nullptr, 0);
  ImuResid o;
#pragma unroll
  for (int i = 0; i < 31; ++i) o.r[i] = t[i];
  return o;
}
// rs [32][64]: entry i of the lane's factor at rs[i * 64 + lane]; row 31 (the kernel's per-factor result) cleared
__device__ __forceinline__ void imu_stage(double *rs, int lane, const ImuResid &v) {
#pragma unroll
  for (int i = 0; i < 31; ++i) rs[i * 64 + lane] = v.r[i];
  rs[31 * 64 + lane] = 0.0;
}
// uq [31] = row `row` of the upper-triangular sqrt_info (row-major 31 x 31), zero left of the diagonal without loading it; then entry
// `row` of sqrt_info r for the factor staged at column fl of rs, terms in ascending order
__device__ __forceinline__ void imu_info_row(const double *sqrt_info, int row, double *uq) {
#pragma unroll
  for (int q = 0; q < 31; ++q) uq[q] = (q >= row) ? sqrt_info[row * 31 + q] : 0.0;
}
__device__ __forceinline__ double imu_row_dot(const double *uq, const double *rs, int fl) {
  double u = 0.0;
#pragma unroll
  for (int q = 0; q < 31; ++q) u += uq[q] * rs[q * 64 + fl];
  return u;
}

// ---- prior part (MarginalizationFactor::Evaluate through H = J0^T J0, b0 = J0^T r0, c0 = r0^T r0: cost 1/2 (dx^T (H dx + 2 b0) + c0)) ----
// block `tid` (< WinMeta::prior_nb) of the window's prior: its part of dxs from the window's state x, by one thread
__device__ __forceinline__ void prior_dx_block(const BatchDev &b, int win, int tid, const double *x, double *dxs) {
  const int bl = win * 40 + tid;
  vilo::prior_dx(x + b.prior_bstate[bl], b.prior_x0 + (size_t)win * 280 + b.prior_bxoff[bl], b.prior_bsize[bl], dxs + b.prior_bidx[bl]);
}
// a row's term of dx^T (H dx + 2 b0); hdx: the row of H dx
__device__ __forceinline__ double prior_row_term(double dx, double hdx, double b0) { return dx * (hdx + 2.0 * b0); }
