// Where a batch's landmarks will be in the next frame's cameras (vilo_batch_predict_next_frame, include/vilo_gpu.h;
// Estimator::predictPtsInNextFrame, estimator.cpp:1694-1727, called by processImage after the solve and the outlier rejection, :811-819).
//
// One launch sequence, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor
// on its position):
//   k_predict_next_frame  one wave per packed visual wave, lane = landmark: k_triangulate's mapping. The window's frame poses and extrinsics
//                         are staged in LDS once per wave. Every lane forms the next pose redundantly (predict_next_pose: a few dozen
//                         flops from the LDS copy, or from the window's row of the uploaded poses), so the window's status is uniform over
//                         the wave and nothing crosses lanes. A lane counts its track's observations in its column of the wave's flag image
//                         (bit 0 of flag[t][n_lanes], t < kmax), tests the selection and carries its first observation's point through the
//                         start frame into the next frame's camera(s). Values go to the caller's landmark order (lm_off + lm_perm); padding
//                         lanes write nothing; a landmark that is not predicted writes zeros.
//   k_predict_windows     64 lanes per window, four windows per workgroup, launched after the first kernel on the same stream: lane 0 forms
//                         the next pose again (the same function on the same values: the same bits) and writes the pose and
//                         the record; the 64 lanes count bit 0 of the window's flags, an integer sum by an xor butterfly (exact in any
//                         order, so no atomics and nothing to order). A window without landmarks has no packed wave and is served here alone.
//
// Floating-point contraction is off for the whole file, the inlined helpers of vilo_math.hpp included: both kernels form the next pose and
// must get the same bits from the same values, whatever code surrounds the inlined body. The call is a few hundred flops per landmark.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "cost_eval.hpp"
#include "lin_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_predict_opts) == 8, "vilo_predict_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_predict_record) == 8, "vilo_window_predict_record: 8 bytes (include/vilo_gpu.h)");

#define PREDICT_WIN_THREADS 256
#define PREDICT_WIN_LANES 64   // lanes of a window in k_predict_windows

struct PredictArgs {
  int mode, right;
  const double *pose_in;              // [W][7] (VILO_PREDICT_GIVEN), else null
  double *pts, *pts_right;            // [n_lm][3] caller order; pts_right may be null
  unsigned char *flags;               // [n_lm] caller order
  double *next_pose;                  // [W][7]
  vilo_window_predict_record *rec;    // [W]
};

namespace {

struct NextPose {
  double pose[7];   // what next_pose reports: px py pz qx qy qz qw
  int status;
};

// The next pose of a window from its frame poses (7 doubles per frame) and extrinsics (two of 7), or from the given row.
__device__ __forceinline__ NextPose predict_next_pose(const double *poses, const double *ex, int n_frames, int mode, int right, const double *given) {
  using namespace vilo;
  NextPose np;
  const int k = n_frames - 1;
  const double *pk = poses + 7 * k;
#pragma unroll
  for (int i = 0; i < 7; ++i) np.pose[i] = pk[i];
  if (mode == VILO_PREDICT_CONSTANT_VELOCITY && n_frames < 3) { np.status = VILO_PREDICT_TOO_FEW_FRAMES; return np; }
  bool finite = true;
  for (int e = 0; e < 7 * n_frames; ++e) finite = finite && isfinite(poses[e]);
  for (int e = 0; e < (right ? 14 : 7); ++e) finite = finite && isfinite(ex[e]);
  double out[7];
  if (mode == VILO_PREDICT_GIVEN) {
    const quat q = qnormalized(ldq_pose(given));
    out[0] = given[0]; out[1] = given[1]; out[2] = given[2];
    out[3] = q.x; out[4] = q.y; out[5] = q.z; out[6] = q.w;
  } else {
    // nextT = curT (prevT^-1 curT): P_n = P_k + R_k R_{k-1}^T (P_k - P_{k-1}), q_n = normalise(q_k (x) q_{k-1}^-1 (x) q_k)
    const double *pp = poses + 7 * (k - 1);
    const quat qk = qnormalized(ldq_pose(pk)), qp = qnormalized(ldq_pose(pp));
    const v3 Pk = ld3(pk), d = Pk - ld3(pp);
    const v3 Pn = Pk + qR(qk) * (tr(qR(qp)) * d);
    const quat q = qnormalized(qmul(qk, qmul(mkq(qp.w, -qp.x, -qp.y, -qp.z), qk)));
    out[0] = Pn.x; out[1] = Pn.y; out[2] = Pn.z;
    out[3] = q.x; out[4] = q.y; out[5] = q.z; out[6] = q.w;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) finite = finite && isfinite(out[i]);
  if (!finite) { np.status = VILO_PREDICT_NUMERIC; return np; }
#pragma unroll
  for (int i = 0; i < 7; ++i) np.pose[i] = out[i];
  np.status = VILO_PREDICT_OK;
  return np;
}

}  // namespace

__global__ void __launch_bounds__(64) k_predict_next_frame(BatchDev b, PredictArgs a) {
  using namespace vilo;
  __shared__ double xs[WIN_XS];
  const WaveMeta wv = b.wave[blockIdx.x];
  const WinMeta wm = b.win[wv.win];
  const int lane = threadIdx.x;
  stage_window_frames(xs, b.x + (size_t)wv.win * XSTRIDE, lane, 64);
  __syncthreads();
  int cs[4], cn[4], ckm[4], cgo[4];
  const LaneSeg ls = lane_segment(wv, b.chunk, lane, cs, cn, ckm, cgo);
  if (!ls.active) return;
  const int n = wv.n_lanes, s = ls.s, gi = ls.gi;
  const size_t o = (size_t)wm.lm_off + b.lm_perm[gi];
  const NextPose np = predict_next_pose(xs, xs + WIN_XS_EX, wm.n_frames, a.mode, a.right, a.pose_in ? a.pose_in + (size_t)7 * wv.win : nullptr);
  // the track's observations: the valid bits of the lane's column are rows 0 .. n_obs - 1
  const unsigned char *flg = b.flags + wv.flag_off;
  int n_obs = 0;
  for (int t = 0; t < wv.kmax; ++t) n_obs += flg[(size_t)t * n + lane] & 1;
  const double lam = b.lam[gi];
  const bool sel = np.status == VILO_PREDICT_OK && lam > 0.0 && n_obs >= 2 && s + n_obs - 1 == wm.n_frames - 1;
  v3 pc = mk3(0.0, 0.0, 0.0), pr = mk3(0.0, 0.0, 0.0);
  unsigned fl = 0;
  if (sel) {
    // everything after the next pose is one path: R_n from the normalised quaternion of the pose that next_pose reports
    const m3 Rn = qR(qnormalized(ldq_pose(np.pose)));
    const v3 Pn = ld3(np.pose);
    const double *obs = b.obs + wv.obs_off;
    const v3 uv0 = mk3(obs_at(obs, n, lane, 0, OBS_LX), obs_at(obs, n, lane, 0, OBS_LY), obs_at(obs, n, lane, 0, OBS_LZ));
    const m3 ric0 = qR(qnormalized(ldq_pose(xs + WIN_XS_EX)));
    const v3 tic0 = ld3(xs + WIN_XS_EX);
    const v3 pts_j = ric0 * (uv0 * (1.0 / lam)) + tic0;
    const v3 pts_w = qR(qnormalized(ldq_pose(xs + 7 * s))) * pts_j + ld3(xs + 7 * s);
    const v3 pts_local = tr(Rn) * (pts_w - Pn);
    pc = tr(ric0) * (pts_local - tic0);
    fl = 1u;
    if (!(pc.z > 0.0)) fl |= 2u;
    bool finite = isfinite(pc.x) && isfinite(pc.y) && isfinite(pc.z);
    if (a.right) {
      const m3 ric1 = qR(qnormalized(ldq_pose(xs + WIN_XS_EX + 7)));
      pr = tr(ric1) * (pts_local - ld3(xs + WIN_XS_EX + 7));
      if (!(pr.z > 0.0)) fl |= 8u;
      finite = finite && isfinite(pr.x) && isfinite(pr.y) && isfinite(pr.z);
    }
    if (!finite) fl |= 4u;
  }
  st3(a.pts + 3 * o, pc);
  if (a.right) st3(a.pts_right + 3 * o, pr);
  a.flags[o] = (unsigned char)fl;
}

__global__ void __launch_bounds__(PREDICT_WIN_THREADS) k_predict_windows(BatchDev b, PredictArgs a) {
  const int win = blockIdx.x * (PREDICT_WIN_THREADS / PREDICT_WIN_LANES) + (threadIdx.x / PREDICT_WIN_LANES), lane = threadIdx.x % PREDICT_WIN_LANES;
  // (a window past the batch's end takes the last window's place and writes nothing: the shuffles below want every lane of the wave)
  const bool win_ok = win < b.W;
  const int wi = win_ok ? win : b.W - 1;
  const WinMeta wm = b.win[wi];
  int cnt = 0;
  for (int l = lane; l < wm.L; l += PREDICT_WIN_LANES) cnt += a.flags[(size_t)wm.lm_off + l] & 1;
#pragma unroll
  for (int off = PREDICT_WIN_LANES / 2; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, PREDICT_WIN_LANES);
  if (!win_ok || lane != 0) return;
  const double *x = b.x + (size_t)wi * XSTRIDE;
  const NextPose np = predict_next_pose(x + XO_POSE, x + XO_EX, wm.n_frames, a.mode, a.right, a.pose_in ? a.pose_in + (size_t)7 * wi : nullptr);
  if (a.next_pose) {
#pragma unroll
    for (int i = 0; i < 7; ++i) a.next_pose[(size_t)7 * wi + i] = np.pose[i];
  }
  vilo_window_predict_record r;
  r.n_predicted = cnt;
  r.status = np.status;
  a.rec[wi] = r;
}

extern "C" void vilo_default_predict_opts(vilo_predict_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->mode = VILO_PREDICT_CONSTANT_VELOCITY;
}

static int predict_check_opts(vilo_ctx *ctx, const vilo_predict_opts *opts, const double *next_pose_in, vilo_predict_opts *o) {
  if (opts) *o = *opts; else vilo_default_predict_opts(o);
  if (o->mode != VILO_PREDICT_CONSTANT_VELOCITY && o->mode != VILO_PREDICT_GIVEN) {
    ctx->err = "vilo_batch_predict_next_frame: mode must be VILO_PREDICT_CONSTANT_VELOCITY or VILO_PREDICT_GIVEN";
    return VILO_ERR_BAD_ARG;
  }
  if (o->mode == VILO_PREDICT_GIVEN && !next_pose_in) {
    ctx->err = "vilo_batch_predict_next_frame: VILO_PREDICT_GIVEN needs next_pose_in";
    return VILO_ERR_BAD_ARG;
  }
  return VILO_OK;
}

extern "C" int vilo_batch_predict_next_frame(vilo_ctx *ctx, vilo_batch *bt, const vilo_predict_opts *opts, const double *next_pose_in, double *pts_cam,
                                             double *pts_cam_right, uint8_t *flags, double *next_pose, vilo_window_predict_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_predict_opts o;
  const int rc = predict_check_opts(ctx, opts, next_pose_in, &o);
  if (rc != VILO_OK) return rc;
  if (bt->mask.refuse(ctx, "vilo_batch_predict_next_frame") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  const BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm;
  if (n_lm > 0 && !pts_cam) {
    ctx->err = "vilo_batch_predict_next_frame: pts_cam is NULL";
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_predict_ms);
  if (W == 0) return VILO_OK;
  const bool given = o.mode == VILO_PREDICT_GIVEN, right = pts_cam_right != nullptr;
  // the call's device memory: points | right-camera points | flags | given poses | next poses | records
  const size_t o_p = call.lay.take<double>(3 * (size_t)n_lm), o_r = call.lay.take<double>(3 * (size_t)n_lm, right);
  const size_t o_f = call.lay.take<unsigned char>(n_lm), o_g = call.lay.take<double>(7 * (size_t)W, given);
  const size_t o_n = call.lay.take<double>(7 * (size_t)W), o_c = call.lay.take<vilo_window_predict_record>(W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  PredictArgs a;
  a.mode = o.mode; a.right = right ? 1 : 0;
  a.pose_in = given ? call.ptr<double>(o_g) : nullptr;
  a.pts = call.ptr<double>(o_p);
  a.pts_right = right ? call.ptr<double>(o_r) : nullptr;
  a.flags = call.ptr<unsigned char>(o_f);
  a.next_pose = call.ptr<double>(o_n);
  a.rec = call.ptr<vilo_window_predict_record>(o_c);
  if (given) VILO_HIP(hipMemcpyAsync(call.ptr<char>(o_g), next_pose_in, sizeof(double) * 7 * (size_t)W, hipMemcpyHostToDevice, ctx->stream));   // (not timed)
  VILO_HIP(call.start());
  if (bd.n_waves > 0) hipLaunchKernelGGL(k_predict_next_frame, dim3(bd.n_waves), dim3(64), 0, ctx->stream, bd, a);
  const int per_block = PREDICT_WIN_THREADS / PREDICT_WIN_LANES;
  hipLaunchKernelGGL(k_predict_windows, dim3((W + per_block - 1) / per_block), dim3(PREDICT_WIN_THREADS), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(pts_cam, a.pts, sizeof(double) * 3 * (size_t)n_lm));
  if (right) VILO_HIP(call.down(pts_cam_right, a.pts_right, sizeof(double) * 3 * (size_t)n_lm));
  VILO_HIP(call.down(flags, a.flags, (size_t)n_lm));
  VILO_HIP(call.down(next_pose, a.next_pose, sizeof(double) * 7 * (size_t)W));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_predict_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_predict_next_frame(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                              const vilo_predict_opts *opts, const double *next_pose_in, double *pts_cam, double *pts_cam_right,
                                              uint8_t *flags, double *next_pose, vilo_window_predict_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_predict_opts o;
  const int rc = predict_check_opts(ctx, opts, next_pose_in, &o);
  if (rc != VILO_OK) return rc;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_predict_next_frame(ctx, bt, &o, next_pose_in, pts_cam, pts_cam_right, flags, next_pose, records);
  });
}

extern "C" double vilo_last_predict_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_predict_ms : -1.0; }
