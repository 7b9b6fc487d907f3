// Pose of one frame per window from the landmarks that have depth (vilo_batch_frame_pose_pnp, include/vilo_gpu.h;
// FeatureManager::initFramePoseByPnP, feature_manager.cpp:259-300, with solvePoseByPnP :215-257 restated as plain Gauss-Newton: parity
// unpinned against OpenCV).
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_frame_pose_pnp  one workgroup of four waves per window, lane = landmark. The window's frame poses and extrinsics are staged in LDS
//                     once. Hardware wave h walks the window's packed visual waves h, h + 4, ... (WinMeta::wave_off, n_waves) with
//                     lane_segment; a lane forms the world point and reads the frame's image point of each landmark it meets once, before
//                     the first iteration: the first trip's stays in registers, the later trips' (a window with more than 256 packed
//                     lanes) in the lane's own slots of dynamic LDS. Per iteration a lane adds its points' 21 + 6 + 1 terms of J^T J,
//                     J^T r, r^T r (trips ascending); the 28 sums are reduced by an xor butterfly inside a wave and through LDS across the
//                     four waves, in wave order, so every lane holds the same bits: no atomics. The 6 x 6 Cholesky, both triangular solves
//                     and the exponential-map update are done redundantly by every lane; the exit tests are therefore uniform. A point
//                     behind the camera poisons r^T r with NaN, which is the uniform NUMERIC test. Thread 0 writes the window's pose and
//                     record, and with `write` the pose row of the batch's current state.
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "cost_eval.hpp"
#include "lin_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_pnp_opts) == 24, "vilo_pnp_opts: 24 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_pnp_record) == 32, "vilo_window_pnp_record: 32 bytes (include/vilo_gpu.h)");

#define PNP_THREADS 256
#define PNP_WAVES 4
#define PNP_NSUM 28        // upper triangle of J^T J (21), J^T r (6), r^T r
#define PNP_PT 5           // world point and image point of a landmark
#define PNP_MAX_TRIPS 7    // VILO_NUM_OF_F landmarks make at most 26 packed waves (15 full chunks + one ragged chunk per start frame)

struct PnpArgs {
  int frame, guess, write, max_iterations;
  double step_tolerance;
  double *pose;                  // [W][7]
  vilo_window_pnp_record *rec;   // [W]
};

namespace {

// sums of v over the workgroup, the same bits in every lane: xor butterfly inside a wave (lanes_sum), then the
// four waves' sums in wave order. red: [PNP_WAVES][N] of LDS, free again when the call returns.
template <int N>
__device__ __forceinline__ void pnp_block_sum(double (&v)[N], double *red, int wave, int lane) {
  lanes_sum<N, 64>(v);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
  __syncthreads();
}

// a point's terms at cam_T_w = (R, t), left-multiplicative perturbation (dtheta, dt): Y = R X + t, residual pi(Y) - uv,
// J = dpi/dY [-[Y]x | I]. A point with Y.z <= 0 contributes NaN to r^T r.
__device__ __forceinline__ void pnp_accumulate(const vilo::m3 &R, const vilo::v3 &t, const double (&p)[PNP_PT], double (&acc)[PNP_NSUM]) {
  using namespace vilo;
  const v3 Y = R * mk3(p[0], p[1], p[2]) + t;
  const double iz = 1.0 / Y.z;
  const double u = Y.x * iz, v = Y.y * iz;
  const double r0 = u - p[3], r1 = v - p[4];
  const double J0[6] = {-u * v, 1.0 + u * u, -v, iz, 0.0, -u * iz};
  const double J1[6] = {-1.0 - v * v, u * v, u, 0.0, iz, -v * iz};
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) acc[e++] += J0[i] * J0[j] + J1[i] * J1[j];
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] += J0[i] * r0 + J1[i] * r1;
  acc[27] += Y.z > 0.0 ? r0 * r0 + r1 * r1 : NAN;
}

// H d = -g by Cholesky (H: packed upper triangle, rows ascending); false: a pivot is not positive
__device__ __forceinline__ bool pnp_solve6(const double (&s)[PNP_NSUM], double (&d)[6]) {
  double L[6][6];
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) L[j][i] = s[e++];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= L[j][k] * L[j][k];
    if (!(dj > 0.0)) ok = false;
    const double lj = sqrt(dj), ilj = 1.0 / lj;
    L[j][j] = lj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double x = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) x -= L[i][k] * L[j][k];
      L[i][j] = x * ilj;
    }
  }
  double y[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double x = -s[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) x -= L[i][k] * y[k];
    y[i] = x / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double x = y[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) x -= L[k][i] * d[k];
    d[i] = x / L[i][i];
  }
  return ok;
}

// Rodrigues' formula; below 1e-4 rad the series to the order that is exact in FP64
__device__ __forceinline__ vilo::m3 pnp_exp(const vilo::v3 &w) {
  using namespace vilo;
  const double th2 = dot(w, w), th = sqrt(th2);
  double a, b;
  if (th < 1e-4) { a = 1.0 - th2 / 6.0; b = 0.5 - th2 / 24.0; }
  else { a = sin(th) / th; b = (1.0 - cos(th)) / th2; }
  const m3 K = skew(w);
  return m3_eye() + K * a + (K * K) * b;
}

// quaternion [x y z w] of a rotation matrix (the branches of Eigen's Quaternion(Matrix3)), normalised, w >= 0
__device__ __forceinline__ void pnp_quat(const vilo::m3 &R, double *q) {
  double x, y, z, w;
  const double tr = R.a[0] + R.a[4] + R.a[8];
  if (tr > 0.0) {
    const double s = sqrt(tr + 1.0), h = 0.5 / s;
    w = 0.5 * s; x = (R.a[7] - R.a[5]) * h; y = (R.a[2] - R.a[6]) * h; z = (R.a[3] - R.a[1]) * h;
  } else if (R.a[0] >= R.a[4] && R.a[0] >= R.a[8]) {
    const double s = sqrt(R.a[0] - R.a[4] - R.a[8] + 1.0), h = 0.5 / s;
    x = 0.5 * s; w = (R.a[7] - R.a[5]) * h; y = (R.a[3] + R.a[1]) * h; z = (R.a[6] + R.a[2]) * h;
  } else if (R.a[4] >= R.a[8]) {
    const double s = sqrt(R.a[4] - R.a[8] - R.a[0] + 1.0), h = 0.5 / s;
    y = 0.5 * s; w = (R.a[2] - R.a[6]) * h; z = (R.a[7] + R.a[5]) * h; x = (R.a[1] + R.a[3]) * h;
  } else {
    const double s = sqrt(R.a[8] - R.a[0] - R.a[4] + 1.0), h = 0.5 / s;
    z = 0.5 * s; w = (R.a[3] - R.a[1]) * h; x = (R.a[2] + R.a[6]) * h; y = (R.a[5] + R.a[7]) * h;
  }
  const double n = sqrt(x * x + y * y + z * z + w * w) * (w < 0.0 ? -1.0 : 1.0);
  q[0] = x / n; q[1] = y / n; q[2] = z / n; q[3] = w / n;
}

}  // namespace

__global__ void __launch_bounds__(PNP_THREADS) k_frame_pose_pnp(BatchDev b, PnpArgs a) {
  using namespace vilo;
  extern __shared__ double pnp_pts[];   // [trip - 1][PNP_PT][PNP_THREADS]: a lane's points of the trips after the first
  __shared__ double xs[WIN_XS];
  __shared__ double red[PNP_WAVES * PNP_NSUM];
  const int win = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const WinMeta wm = b.win[win];
  stage_window_frames(xs, b.x + (size_t)win * XSTRIDE, tid, PNP_THREADS);
  __syncthreads();
  const int k = a.frame < 0 ? wm.n_frames - 1 : a.frame;   // (the host keeps a.frame <= VILO_MAX_FRAMES - 1: row k of xs exists)
  const bool frame_ok = k >= 1 && k <= wm.n_frames - 1;
  const m3 ric0 = qR(qnormalized(ldq_pose(xs + WIN_XS_EX)));
  const v3 tic0 = ld3(xs + WIN_XS_EX);

  // ---- the points: once, before the first iteration ----
  const int n_trips = frame_ok ? min((wm.n_waves + PNP_WAVES - 1) / PNP_WAVES, PNP_MAX_TRIPS) : 0;
  double p0[PNP_PT] = {0.0, 0.0, 0.0, 0.0, 0.0};
  unsigned used = 0;   // bit `trip`: this lane has a point there
#pragma unroll 1
  for (int trip = 0; trip < n_trips; ++trip) {
    const int j = trip * PNP_WAVES + wave;
    double p[PNP_PT] = {0.0, 0.0, 0.0, 0.0, 0.0};
    bool use = false;
    if (j < wm.n_waves) {
      const WaveMeta wv = b.wave[wm.wave_off + j];
      int cs[4], cn[4], ckm[4], cgo[4];
      const LaneSeg ls = lane_segment(wv, b.chunk, lane, cs, cn, ckm, cgo);
      const int t = k - ls.s, n = wv.n_lanes;
      if (ls.active && t >= 1 && t < wv.kmax && (b.flags[wv.flag_off + (size_t)t * n + lane] & 1)) {
        const double lam = b.lam[ls.gi];
        if (lam > 0.0) {
          const double *obs = b.obs + wv.obs_off;
          const v3 pt0 = mk3(obs_at(obs, n, lane, 0, OBS_LX), obs_at(obs, n, lane, 0, OBS_LY), obs_at(obs, n, lane, 0, OBS_LZ));
          const double *pose_s = xs + 7 * ls.s;
          const v3 X = qR(qnormalized(ldq_pose(pose_s))) * (ric0 * (pt0 * (1.0 / lam)) + tic0) + ld3(pose_s);
          p[0] = X.x; p[1] = X.y; p[2] = X.z;
          p[3] = obs_at(obs, n, lane, t, OBS_LX);
          p[4] = obs_at(obs, n, lane, t, OBS_LY);
          use = true;
        }
      }
    }
    if (use) used |= 1u << trip;
    if (trip == 0) {
#pragma unroll
      for (int c = 0; c < PNP_PT; ++c) p0[c] = p[c];
    } else {
#pragma unroll
      for (int c = 0; c < PNP_PT; ++c) pnp_pts[((size_t)(trip - 1) * PNP_PT + c) * PNP_THREADS + tid] = p[c];
    }
  }
  double cnt[1] = {(double)__popc(used)};
  pnp_block_sum<1>(cnt, red, wave, lane);
  const int n_points = (int)cnt[0];

  // ---- the start: w_T_cam of the previous frame (or of frame k), inverted ----
  const int kc = frame_ok ? k : 1;
  const double *pose_g = xs + 7 * (a.guess == VILO_PNP_GUESS_CURRENT ? kc : kc - 1);
  m3 R;
  v3 t;
  {
    const m3 Rg = qR(qnormalized(ldq_pose(pose_g)));
    const m3 RCam = Rg * ric0;
    const v3 PCam = Rg * tic0 + ld3(pose_g);
    R = tr(RCam);
    t = -(R * PCam);
  }

  int status = VILO_PNP_OK, iterations = 0;
  double cost = 0.0, initial_cost = 0.0;
  if (!frame_ok) status = VILO_PNP_NO_FRAME;
  else if (n_points < 4) status = VILO_PNP_NOT_ENOUGH_POINTS;
  else {
    bool converged = false;
    for (;;) {
      double acc[PNP_NSUM];
#pragma unroll
      for (int i = 0; i < PNP_NSUM; ++i) acc[i] = 0.0;
#pragma unroll 1
      for (int trip = 0; trip < n_trips; ++trip)
        if (used & (1u << trip)) {
          double p[PNP_PT];
#pragma unroll
          for (int c = 0; c < PNP_PT; ++c) p[c] = trip == 0 ? p0[c] : pnp_pts[((size_t)(trip - 1) * PNP_PT + c) * PNP_THREADS + tid];
          pnp_accumulate(R, t, p, acc);
        }
      pnp_block_sum<PNP_NSUM>(acc, red, wave, lane);
      cost = 0.5 * acc[27];
      if (iterations == 0) initial_cost = cost;
      if (!isfinite(cost)) { status = VILO_PNP_NUMERIC; break; }
      if (converged) break;
      if (iterations == a.max_iterations) { status = VILO_PNP_NO_CONVERGENCE; break; }
      double d[6];
      const bool pd = pnp_solve6(acc, d);
      double n2 = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) n2 += d[i] * d[i];
      if (!pd || !isfinite(n2)) { status = VILO_PNP_NUMERIC; break; }
      const m3 E = pnp_exp(mk3(d[0], d[1], d[2]));
      R = E * R;
      t = E * t + mk3(d[3], d[4], d[5]);
      ++iterations;
      converged = sqrt(n2) <= a.step_tolerance;
    }
  }

  if (tid == 0) {
    double out[7];
    if (status == VILO_PNP_OK || status == VILO_PNP_NO_CONVERGENCE) {
      // cam_T_w -> w_T_cam -> w_T_imu (:253-254, :292-293)
      const m3 RCam = tr(R);
      const v3 PCam = -(RCam * t);
      const m3 Rk = RCam * tr(ric0);
      const v3 Pk = PCam - Rk * tic0;
      out[0] = Pk.x; out[1] = Pk.y; out[2] = Pk.z;
      pnp_quat(Rk, out + 3);
    } else {
#pragma unroll
      for (int i = 0; i < 7; ++i) out[i] = xs[7 * k + i];   // the frame's current pose, bit for bit
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) a.pose[(size_t)7 * win + i] = out[i];
    vilo_window_pnp_record r;
    r.final_cost = cost; r.initial_cost = initial_cost;
    r.n_points = n_points; r.iterations = iterations; r.status = status; r.pad = 0;
    a.rec[win] = r;
    if (a.write && status == VILO_PNP_OK) {
      double *x = b.x + (size_t)win * XSTRIDE + XO_POSE + 7 * k;
#pragma unroll
      for (int i = 0; i < 7; ++i) x[i] = out[i];
    }
  }
}

extern "C" void vilo_default_pnp_opts(vilo_pnp_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->frame = -1;
  o->guess = VILO_PNP_GUESS_PREVIOUS;
  o->write = 0;
  o->max_iterations = 20;
  o->step_tolerance = 1e-12;
}

static int pnp_check_opts(vilo_ctx *ctx, const vilo_pnp_opts *opts, vilo_pnp_opts *o) {
  if (opts) *o = *opts; else vilo_default_pnp_opts(o);
  if (o->guess != VILO_PNP_GUESS_PREVIOUS && o->guess != VILO_PNP_GUESS_CURRENT) {
    ctx->err = "vilo_batch_frame_pose_pnp: guess must be VILO_PNP_GUESS_PREVIOUS or VILO_PNP_GUESS_CURRENT";
    return VILO_ERR_BAD_ARG;
  }
  if (o->frame < -1 || o->frame == 0 || o->frame > VILO_MAX_FRAMES - 1) {
    ctx->err = "vilo_batch_frame_pose_pnp: frame must be -1 (the last frame) or 1 .. VILO_MAX_FRAMES - 1";
    return VILO_ERR_BAD_ARG;
  }
  if (o->max_iterations < 1 || o->max_iterations > 64) {
    ctx->err = "vilo_batch_frame_pose_pnp: max_iterations must be 1 .. 64";
    return VILO_ERR_BAD_ARG;
  }
  if (!isfinite(o->step_tolerance) || o->step_tolerance < 0.0) {
    ctx->err = "vilo_batch_frame_pose_pnp: step_tolerance must be finite and not negative";
    return VILO_ERR_BAD_ARG;
  }
  return VILO_OK;
}

extern "C" int vilo_batch_frame_pose_pnp(vilo_ctx *ctx, vilo_batch *bt, const vilo_pnp_opts *opts, double *pose, vilo_window_pnp_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_pnp_opts o;
  const int rc = pnp_check_opts(ctx, opts, &o);
  if (rc != VILO_OK) return rc;
  if (bt->mask.refuse(ctx, "vilo_batch_frame_pose_pnp") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  BatchDev &bd = bt->d;
  const int W = bd.W;
  if (W > 0 && !pose) {
    ctx->err = "vilo_batch_frame_pose_pnp: pose is NULL";
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_pnp_ms);
  if (W == 0) return VILO_OK;
  // a lane's points beyond its first live in LDS: one slot per further trip over the window's packed waves
  const int trips = (bt->lm.max_win_waves + PNP_WAVES - 1) / PNP_WAVES;
  if (trips > PNP_MAX_TRIPS) {
    ctx->err = "vilo_batch_frame_pose_pnp: a window has more packed waves than VILO_NUM_OF_F landmarks can make";
    return VILO_ERR_UNSUPPORTED;
  }
  const size_t lds_bytes = sizeof(double) * PNP_PT * PNP_THREADS * (size_t)(trips > 1 ? trips - 1 : 0);
  const size_t o_p = call.lay.take<double>(7 * (size_t)W), o_r = call.lay.take<vilo_window_pnp_record>(W);   // the call's device memory: poses | records
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  PnpArgs a;
  a.frame = o.frame; a.guess = o.guess; a.write = o.write ? 1 : 0; a.max_iterations = o.max_iterations;
  a.step_tolerance = o.step_tolerance;
  a.pose = call.ptr<double>(o_p);
  a.rec = call.ptr<vilo_window_pnp_record>(o_r);
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_frame_pose_pnp, dim3(W), dim3(PNP_THREADS), lds_bytes, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(pose, a.pose, sizeof(double) * 7 * (size_t)W));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_pnp_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_frame_pose_pnp(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                                          const vilo_pnp_opts *opts, double *pose, vilo_window_pnp_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_pnp_opts o;
  const int rc = pnp_check_opts(ctx, opts, &o);
  if (rc != VILO_OK) return rc;
  if (!pose) {
    ctx->err = "vilo_window_frame_pose_pnp: pose is NULL";
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_frame_pose_pnp(ctx, bt, &o, pose, records);
    if (r != VILO_OK || !o.write) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);   // (the other state arrays come back as they went up)
  });
}

extern "C" double vilo_last_pnp_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_pnp_ms : -1.0; }
