// Depths of a batch's landmarks from its current poses and the first two observation rows (vilo_batch_triangulate, include/vilo_gpu.h;
// FeatureManager::triangulate, feature_manager.cpp:302-382 with triangulatePoint :198-212, and the arithmetic of
// FeatureManager::removeBackShiftDepth :450-479).
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_triangulate  one wave per packed visual wave, lane = landmark. The window's frame poses and extrinsics are staged in LDS once per
//                  wave; a lane reads rows t = 0 and t = 1 of the wave's observation image, forms the two 3 x 4 camera matrices
//                  [R0^T | -R0^T t0] of its branch (stereo: left / right camera of the start frame; two-frame: left camera of the start
//                  frame and of the next), builds triangulatePoint's 4 x 4 design matrix and takes the right singular vector of its
//                  smallest singular value by one-sided Jacobi — smallest_right_singular_vector4 of host/vilo_feature_window.cpp, the
//                  (p, q) pairs unrolled so that both 4 x 4 matrices stay in registers. A lane leaves the sweep loop when its own
//                  off-diagonal measure is below the threshold. Values go to the caller's landmark order (lm_off + lm_perm); padding
//                  lanes write nothing. With `write` the lane stores 1 / depth into the batch's current inverse depths (its own entry:
//                  no atomics).
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "cost_eval.hpp"
#include "lin_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_triangulate_opts) == 24, "vilo_triangulate_opts: 24 bytes (include/vilo_gpu.h)");

#define TRI_SWEEPS 60       // sweep limit of the one-sided Jacobi iteration
#define TRI_OFF_TOL 1e-15   // a lane stops when max |u_p . u_q| / (|u_p| |u_q|) of a sweep is below this

struct TriArgs {
  double init_depth;
  int stereo, select, write;
  const unsigned char *mask;   // [n_lm] caller order (VILO_TRI_MASK), else null
  double *depth;               // [n_lm] caller order
  double *shift;               // [n_lm] caller order, or null
  unsigned char *flags;        // [n_lm] caller order
};

namespace {

// the 3 x 4 projection [R^T | -R^T t] of camera (ric, tic) on body pose (Rs, Ps) (feature_manager.cpp:312-325); R and t are returned too
struct TriCam {
  vilo::m3 R, Rt;
  vilo::v3 t, mt;
};
__device__ __forceinline__ TriCam tri_camera(const vilo::m3 &Rs, const vilo::v3 &Ps, const vilo::m3 &ric, const vilo::v3 &tic) {
  using namespace vilo;
  TriCam c;
  c.t = Ps + Rs * tic;
  c.R = Rs * ric;
  c.Rt = tr(c.R);
  c.mt = -(c.Rt * c.t);
  return c;
}

// one rotation of columns P, Q (compile-time: every array index below is a constant once the callers' loops are unrolled)
template <int P, int Q>
__device__ __forceinline__ void tri_rotate(double (&U)[16], double (&V)[16], double &off) {
  double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { al += U[4 * i + P] * U[4 * i + P]; be += U[4 * i + Q] * U[4 * i + Q]; ga += U[4 * i + P] * U[4 * i + Q]; }
  if (ga == 0.0) return;
  off = fmax(off, fabs(ga) / sqrt(al * be + 1e-300));
  const double zeta = (be - al) / (2.0 * ga);
  const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const double up = U[4 * i + P], uq = U[4 * i + Q];
    U[4 * i + P] = c * up - s * uq; U[4 * i + Q] = s * up + c * uq;
    const double vp = V[4 * i + P], vq = V[4 * i + Q];
    V[4 * i + P] = c * vp - s * vq; V[4 * i + Q] = s * vp + c * vq;
  }
}

// right singular vector of the smallest singular value of the 4 x 4 matrix U (overwritten): one-sided Jacobi on its columns
__device__ __forceinline__ void tri_smallest_right_singular_vector4(double (&U)[16], double (&v)[4]) {
  double V[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
#pragma unroll 1
  for (int sweep = 0; sweep < TRI_SWEEPS; ++sweep) {
    double off = 0.0;
    tri_rotate<0, 1>(U, V, off); tri_rotate<0, 2>(U, V, off); tri_rotate<0, 3>(U, V, off);
    tri_rotate<1, 2>(U, V, off); tri_rotate<1, 3>(U, V, off); tri_rotate<2, 3>(U, V, off);
    if (off < TRI_OFF_TOL) break;
  }
  double smin = 1e300;
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = V[4 * i];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double s2 = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s2 += U[4 * i + j] * U[4 * i + j];
    if (s2 < smin) {
      smin = s2;
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = V[4 * i + j];
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(64) k_triangulate(BatchDev b, TriArgs a) {
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
  const int n = wv.n_lanes, s = ls.s, gi = ls.gi, o = wm.lm_off + b.lm_perm[gi];
  const double *obs = b.obs + wv.obs_off;
  const unsigned char *flg = b.flags + wv.flag_off;
  const double lam = b.lam[gi];
  const unsigned char f0 = flg[lane];
  const bool two_views = wv.kmax > 1 && (flg[(size_t)n + lane] & 1);   // (row t = 1 exists only in a wave with kmax > 1)
  const bool st = a.stereo && (f0 & 2);
  bool sel = a.select == 1 ? true : (a.select == 2 ? a.mask[o] != 0 : !(lam > 0.0));
  if (!st && !two_views) sel = false;   // a single mono observation: nothing to triangulate with (the reference leaves its depth alone)
  const v3 uv0 = mk3(obs_at(obs, n, lane, 0, OBS_LX), obs_at(obs, n, lane, 0, OBS_LY), obs_at(obs, n, lane, 0, OBS_LZ));
  const int j = min(s + 1, VILO_MAX_FRAMES - 1);
  const m3 ric0 = qR(qnormalized(ldq_pose(xs + WIN_XS_EX)));
  const v3 tic0 = ld3(xs + WIN_XS_EX);
  const TriCam c0 = tri_camera(qR(qnormalized(ldq_pose(xs + 7 * s))), ld3(xs + 7 * s), ric0, tic0);
  double depth = 1.0 / lam;
  unsigned fl = 0;
  if (sel) {
    // second view: the right camera on the start frame, or the left camera on the next frame
    const double *pose1 = xs + 7 * (st ? s : j), *ex1 = xs + WIN_XS_EX + (st ? 7 : 0);
    const TriCam c1 = tri_camera(qR(qnormalized(ldq_pose(pose1))), ld3(pose1), qR(qnormalized(ldq_pose(ex1))), ld3(ex1));
    const double p1x = st ? obs_at(obs, n, lane, 0, OBS_RX) : obs_at(obs, n, lane, 1, OBS_LX);
    const double p1y = st ? obs_at(obs, n, lane, 0, OBS_RY) : obs_at(obs, n, lane, 1, OBS_LY);
    double U[16], v[4];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      U[c] = uv0.x * c0.Rt.a[6 + c] - c0.Rt.a[c];
      U[4 + c] = uv0.y * c0.Rt.a[6 + c] - c0.Rt.a[3 + c];
      U[8 + c] = p1x * c1.Rt.a[6 + c] - c1.Rt.a[c];
      U[12 + c] = p1y * c1.Rt.a[6 + c] - c1.Rt.a[3 + c];
    }
    U[3] = uv0.x * c0.mt.z - c0.mt.x;
    U[7] = uv0.y * c0.mt.z - c0.mt.y;
    U[11] = p1x * c1.mt.z - c1.mt.x;
    U[15] = p1y * c1.mt.z - c1.mt.y;
    tri_smallest_right_singular_vector4(U, v);
    const double X0 = v[0] / v[3], X1 = v[1] / v[3], X2 = v[2] / v[3];
    const double z = c0.Rt.a[6] * X0 + c0.Rt.a[7] * X1 + c0.Rt.a[8] * X2 + c0.mt.z;   // localPoint.z()
    fl = 1u | (st ? 2u : 0u);
    if (!isfinite(z)) fl |= 8u;
    if (z > 0) depth = z;
    else { depth = a.init_depth; fl |= 4u; }
  }
  const double lam_out = (sel && a.write) ? 1.0 / depth : lam;
  a.depth[o] = depth;
  a.flags[o] = (unsigned char)fl;
  if (sel && a.write) b.lam[gi] = lam_out;
  if (a.shift) {
    double sh = lam_out;
    if (s == 0) {
      // removeBackShiftDepth: marg pose = left camera of frame 0 (c0), new pose = left camera of frame 1
      const TriCam cn1 = tri_camera(qR(qnormalized(ldq_pose(xs + 7))), ld3(xs + 7), ric0, tic0);
      const v3 pts_i = uv0 * (1.0 / lam_out);
      const v3 w_pts_i = c0.R * pts_i + c0.t;
      const v3 pts_j = cn1.Rt * (w_pts_i - cn1.t);
      sh = pts_j.z > 0 ? 1.0 / pts_j.z : 1.0 / a.init_depth;
    }
    a.shift[o] = sh;
  }
}

extern "C" void vilo_default_triangulate_opts(vilo_triangulate_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->init_depth = 5.0;
  o->stereo = 1;
  o->select = VILO_TRI_UNSET;
  o->write = 0;
}

static int tri_check_opts(vilo_ctx *ctx, const vilo_triangulate_opts *opts, const uint8_t *mask, vilo_triangulate_opts *o) {
  if (opts) *o = *opts; else vilo_default_triangulate_opts(o);
  if (!isfinite(o->init_depth) || !(o->init_depth > 0.0)) {
    ctx->err = "vilo_batch_triangulate: init_depth must be finite and > 0";
    return VILO_ERR_BAD_ARG;
  }
  if (o->select != VILO_TRI_UNSET && o->select != VILO_TRI_ALL && o->select != VILO_TRI_MASK) {
    ctx->err = "vilo_batch_triangulate: select must be VILO_TRI_UNSET, VILO_TRI_ALL or VILO_TRI_MASK";
    return VILO_ERR_BAD_ARG;
  }
  if (o->select == VILO_TRI_MASK && !mask) {
    ctx->err = "vilo_batch_triangulate: VILO_TRI_MASK needs a mask";
    return VILO_ERR_BAD_ARG;
  }
  return VILO_OK;
}

extern "C" int vilo_batch_triangulate(vilo_ctx *ctx, vilo_batch *bt, const vilo_triangulate_opts *opts, const uint8_t *mask, double *depth,
                                      uint8_t *flags, double *shift_inv_depth) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_triangulate_opts o;
  int rc = tri_check_opts(ctx, opts, mask, &o);
  if (rc != VILO_OK) return rc;
  if (bt->mask.refuse(ctx, "vilo_batch_triangulate") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  BatchDev &bd = bt->d;
  const int n_lm = bd.n_lm;
  if (n_lm > 0 && !depth) {
    ctx->err = "vilo_batch_triangulate: depth is NULL";
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_tri_ms);
  if (n_lm == 0 || bd.n_waves == 0) return VILO_OK;   // nothing to report: the caller's arrays are not touched
  const bool masked = o.select == VILO_TRI_MASK;
  // the call's device memory: depths | shifted inverse depths | flags | mask
  const size_t o_d = call.lay.take<double>(n_lm), o_s = call.lay.take<double>(n_lm, shift_inv_depth != nullptr);
  const size_t o_f = call.lay.take<unsigned char>(n_lm), o_m = call.lay.take<unsigned char>(n_lm, masked);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  TriArgs a;
  a.init_depth = o.init_depth; a.stereo = o.stereo ? 1 : 0; a.select = o.select; a.write = o.write ? 1 : 0;
  a.mask = masked ? call.ptr<unsigned char>(o_m) : nullptr;
  a.depth = call.ptr<double>(o_d);
  a.shift = shift_inv_depth ? call.ptr<double>(o_s) : nullptr;
  a.flags = call.ptr<unsigned char>(o_f);
  if (masked) VILO_HIP(hipMemcpyAsync(call.ptr<char>(o_m), mask, (size_t)n_lm, hipMemcpyHostToDevice, ctx->stream));   // (not timed)
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_triangulate, dim3(bd.n_waves), dim3(64), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(depth, a.depth, sizeof(double) * (size_t)n_lm));
  VILO_HIP(call.down(flags, a.flags, (size_t)n_lm));
  VILO_HIP(call.down(shift_inv_depth, a.shift, sizeof(double) * (size_t)n_lm));
  return VILO_OK;
}

extern "C" int vilo_window_triangulate(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                                       const vilo_triangulate_opts *opts, const uint8_t *mask, double *depth, uint8_t *flags,
                                       double *shift_inv_depth) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_triangulate_opts o;
  const int rc = tri_check_opts(ctx, opts, mask, &o);
  if (rc != VILO_OK) return rc;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_triangulate(ctx, bt, &o, mask, depth, flags, shift_inv_depth);
    if (r != VILO_OK || !o.write) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);   // (the other state arrays come back as they went up)
  });
}

extern "C" double vilo_last_triangulate_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_tri_ms : -1.0; }
