// double2vector's gauge fix (estimator.cpp:903-957) on gfx950: vilo_gauge_fix on host arrays, vilo_gauge_fix_batch inside
// vilo_optimize_windows, and vilo_batch_gauge_fix / vilo_window_gauge_fix in place on a resident batch, checked and with records.
#include "batch_call.hpp"

using namespace vilo;

namespace {

__device__ v3 R2ypr_deg(const m3 &R) {
  const v3 nn = mk3(R.a[0], R.a[3], R.a[6]), o = mk3(R.a[1], R.a[4], R.a[7]), a = mk3(R.a[2], R.a[5], R.a[8]);
  const double y = atan2(nn.y, nn.x);
  const double p = atan2(-nn.z, nn.x * cos(y) + nn.y * sin(y));
  const double r = atan2(a.x * sin(y) - a.y * cos(y), -o.x * sin(y) + o.y * cos(y));
  return mk3(y / M_PI * 180.0, p / M_PI * 180.0, r / M_PI * 180.0);   // `ypr / M_PI * 180.0` as utility.h:98 writes it (an ulp from `* (180 / pi)`)
}
// what a window's fix reports (vilo_window_gauge_record)
struct GaugeInfo { double yaw_diff_deg; int singular, numeric; };

// One workgroup per window, thread t < F frame t, threads F and F + 1 the two extrinsics. check: a value read that is not finite leaves
// the window unwritten (numeric = 1); write_ex: the extrinsic quaternions are rewritten normalised; p0_out: [7] the solved frame-0 pose.
// vilo_gauge_fix and vilo_optimize_windows run it with check = false and write_ex = true, as they always have.
__device__ GaugeInfo k_gauge_fix_body(int F, const double *bp /*[7]*/, double *pw /*[F][7]*/, double *sw /*[F][9]*/, double *exw /*[2][7]*/, bool check,
                                      bool write_ex, double *p0_out) {
  const int t = threadIdx.x;
  const m3 Rs0 = qR(ldq_pose(bp));
  const m3 R00 = qR(ldq_pose(pw));
  const v3 o0 = R2ypr_deg(Rs0), o00 = R2ypr_deg(R00);
  const double yd = (o0.x - o00.x) / 180.0 * M_PI;
  m3 rot = m3_eye();
  rot.a[0] = cos(yd); rot.a[1] = -sin(yd); rot.a[3] = sin(yd); rot.a[4] = cos(yd);
  const bool singular = fabs(fabs(o0.y) - 90) < 1.0 || fabs(fabs(o00.y) - 90) < 1.0;
  if (singular) rot = Rs0 * tr(R00);
  const v3 P0 = ld3(pw), origin = ld3(bp);
  bool bad = false;
  if (check)
    for (int k = 0; k < 7; ++k) bad = bad || !isfinite(bp[k]) || !isfinite(pw[k]);
  if (p0_out && t == 0)
    for (int k = 0; k < 7; ++k) p0_out[k] = pw[k];
  v3 Pi = P0, Vi = P0;
  quat q = mkq(1.0, 0.0, 0.0, 0.0);
  if (t < F) {
    const double *pp = pw + 7 * t, *ss = sw + 9 * t;
    if (check) {
      for (int k = 0; k < 7; ++k) bad = bad || !isfinite(pp[k]);
      for (int k = 0; k < 3; ++k) bad = bad || !isfinite(ss[k]);
    }
    const m3 Ri = rot * qR(qnormalized(ldq_pose(pp)));
    Pi = rot * (ld3(pp) - P0) + origin;
    Vi = rot * ld3(ss);
    q = quat_from_R_dev(Ri);
  } else if (t < F + 2 && write_ex) {
    const double *pp = exw + 7 * (t - F);
    if (check)
      for (int k = 3; k < 7; ++k) bad = bad || !isfinite(pp[k]);
    q = quat_from_R_dev(qR(qnormalized(ldq_pose(pp))));
  }
  // every read of the window is done before its first write
  const int numeric = __syncthreads_or(check && bad);
  GaugeInfo info;
  info.yaw_diff_deg = numeric ? 0.0 : o0.x - o00.x;
  info.singular = !numeric && singular;
  info.numeric = numeric != 0;
  if (numeric) return info;
  if (t < F) {
    double *pp = pw + 7 * t, *ss = sw + 9 * t;
    st3(pp, Pi);
    pp[3] = q.x; pp[4] = q.y; pp[5] = q.z; pp[6] = q.w;
    st3(ss, Vi);
  } else if (t < F + 2 && write_ex) {
    double *pp = exw + 7 * (t - F);
    pp[3] = q.x; pp[4] = q.y; pp[5] = q.z; pp[6] = q.w;
  }
  return info;
}

__global__ void k_gauge_fix(int W, int F, const double *before_pose0 /*[W][7]*/, double *pose /*[W][F][7]*/, double *sb /*[W][F][9]*/,
                            double *ex /*[W][2][7]*/) {
  const int w = blockIdx.x;
  if (w >= W) return;
  k_gauge_fix_body(F, before_pose0 + 7 * w, pose + (size_t)w * F * 7, sb + (size_t)w * F * 9, ex + (size_t)w * 14, false, true, nullptr);
}

// the same on the state block of a device-resident batch (pose [F][7] at XO_POSE, speed/bias [F][9] at XO_SB, extrinsics at XO_EX).
// anchor null: Rs[0] / Ps[0] of before the solve come from the batch's uploaded initial states. vilo_optimize_windows launches it with
// query = 0: no check, every extrinsic quaternion rewritten, nothing reported; vilo_batch_gauge_fix with query = 1: checked, a constant
// extrinsic block left as uploaded, records and the replaced frame-0 poses where asked for.
struct GaugeArgs {
  const double *anchor;                 // [W][7], or null
  vilo_window_gauge_record *rec;        // [W], or null
  double *pose0_before;                 // [W][7], or null
  int query;
};
__global__ void __launch_bounds__(64) k_gauge_fix_x(BatchDev b, GaugeArgs a) {
  const int w = blockIdx.x;
  double *x = b.x + (size_t)w * XSTRIDE;
  const bool write_ex = !(a.query && (b.win[w].const_mask & CONST_EX));
  const GaugeInfo info = k_gauge_fix_body(b.win[w].n_frames, a.anchor ? a.anchor + 7 * (size_t)w : b.x0 + (size_t)w * XSTRIDE + XO_POSE, x + XO_POSE, x + XO_SB,
                                          x + XO_EX, a.query != 0, write_ex, a.pose0_before ? a.pose0_before + 7 * (size_t)w : nullptr);
  if (a.rec && threadIdx.x == 0) {
    vilo_window_gauge_record r;
    r.yaw_diff_deg = info.yaw_diff_deg;
    r.singular = info.singular;
    r.status = info.numeric ? VILO_GAUGE_NUMERIC : VILO_GAUGE_OK;
    a.rec[w] = r;
  }
}

}  // namespace

int vilo_gauge_fix_batch(vilo_ctx *ctx, BatchDev &bd) {
  GaugeArgs a;
  a.anchor = nullptr; a.rec = nullptr; a.pose0_before = nullptr; a.query = 0;
  hipLaunchKernelGGL(k_gauge_fix_x, dim3(bd.W), dim3(64), 0, ctx->stream, bd, a);
  VILO_HIP(hipGetLastError());
  return VILO_OK;
}

static_assert(sizeof(vilo_gauge_opts) == 8, "vilo_gauge_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_gauge_record) == 16, "vilo_window_gauge_record: 16 bytes (include/vilo_gpu.h)");

extern "C" void vilo_default_gauge_opts(vilo_gauge_opts *o) {
  if (!o) return;
  o->anchor = VILO_GAUGE_ANCHOR_UPLOADED;
  o->reserved = 0;
}

// what is wrong with a gauge-fix call's arguments, or null
static const char *gauge_check(const vilo_gauge_opts &o, const double *anchor_pose) {
  if (o.anchor != VILO_GAUGE_ANCHOR_UPLOADED && o.anchor != VILO_GAUGE_ANCHOR_GIVEN) return "vilo_batch_gauge_fix: anchor must be VILO_GAUGE_ANCHOR_UPLOADED or VILO_GAUGE_ANCHOR_GIVEN";
  if (o.anchor == VILO_GAUGE_ANCHOR_GIVEN && !anchor_pose) return "vilo_batch_gauge_fix: VILO_GAUGE_ANCHOR_GIVEN needs anchor_pose";
  if (o.anchor != VILO_GAUGE_ANCHOR_GIVEN && anchor_pose) return "vilo_batch_gauge_fix: anchor_pose needs VILO_GAUGE_ANCHOR_GIVEN";
  return nullptr;
}

// double2vector's gauge fix (estimator.cpp:903-1003) in place on a resident batch's device state
extern "C" int vilo_batch_gauge_fix(vilo_ctx *ctx, vilo_batch *bt, const vilo_gauge_opts *opts, const double *anchor_pose, vilo_window_gauge_record *records,
                                    double *pose0_before) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_gauge_opts o;
  if (opts) o = *opts; else vilo_default_gauge_opts(&o);
  if (const char *what = gauge_check(o, anchor_pose)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  BatchCall call(ctx, bt, &vilo_ctx::last_gauge_fix_ms);
  if (W == 0) return VILO_OK;
  const bool given = o.anchor == VILO_GAUGE_ANCHOR_GIVEN;
  // the call's device memory: anchor poses | records | replaced frame-0 poses
  const size_t o_a = call.lay.take<double>(7 * (size_t)W, given), o_r = call.lay.take<vilo_window_gauge_record>(W),
               o_p = call.lay.take<double>(7 * (size_t)W, pose0_before != nullptr);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  GaugeArgs a;
  a.anchor = given ? call.ptr<double>(o_a) : nullptr;
  a.rec = call.ptr<vilo_window_gauge_record>(o_r);
  a.pose0_before = pose0_before ? call.ptr<double>(o_p) : nullptr;
  a.query = 1;
  // (not timed)
  if (given) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_a), anchor_pose, sizeof(double) * 7 * (size_t)W, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_gauge_fix_x, dim3(W), dim3(64), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_gauge_record) * (size_t)W));
  VILO_HIP(call.down(pose0_before, a.pose0_before, sizeof(double) * 7 * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_gauge_fix(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_gauge_opts *opts,
                                     const double *anchor_pose, vilo_window_gauge_record *records, double *pose0_before) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_gauge_opts o;
  if (opts) o = *opts; else vilo_default_gauge_opts(&o);
  if (const char *what = gauge_check(o, anchor_pose)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_gauge_fix(ctx, bt, &o, anchor_pose, records, pose0_before);
    if (r != VILO_OK) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);   // (the other state arrays come back as they went up)
  });
}

extern "C" double vilo_last_gauge_fix_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_gauge_fix_ms : -1.0; }

extern "C" int vilo_gauge_fix(vilo_ctx *ctx, int W, const vilo_window_state *before, vilo_window_state *after, int F) {
  if (!ctx || W <= 0 || !before || !after || F < 1 || F > VILO_MAX_FRAMES) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  std::vector<double> bp((size_t)W * 7), pose((size_t)W * F * 7), sb((size_t)W * F * 9), ex((size_t)W * 14);
  for (int w = 0; w < W; ++w) {
    memcpy(&bp[(size_t)w * 7], before[w].pose, 7 * sizeof(double));
    memcpy(&pose[(size_t)w * F * 7], after[w].pose, sizeof(double) * F * 7);
    memcpy(&sb[(size_t)w * F * 9], after[w].speed_bias, sizeof(double) * F * 9);
    memcpy(&ex[(size_t)w * 14], after[w].ex_pose, sizeof(double) * 14);
  }
  DevBuf d_bp, d_pose, d_sb, d_ex;
  VILO_HIP(d_bp.alloc(bp.size() * 8)); VILO_HIP(d_pose.alloc(pose.size() * 8)); VILO_HIP(d_sb.alloc(sb.size() * 8)); VILO_HIP(d_ex.alloc(ex.size() * 8));
  VILO_HIP(hipMemcpyAsync(d_bp.p, bp.data(), bp.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(hipMemcpyAsync(d_pose.p, pose.data(), pose.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(hipMemcpyAsync(d_sb.p, sb.data(), sb.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(hipMemcpyAsync(d_ex.p, ex.data(), ex.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  hipLaunchKernelGGL(k_gauge_fix, dim3(W), dim3(64), 0, ctx->stream, W, F, d_bp.as<double>(), d_pose.as<double>(), d_sb.as<double>(), d_ex.as<double>());
  VILO_HIP(hipGetLastError());
  VILO_HIP(hipMemcpyAsync(pose.data(), d_pose.p, pose.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  VILO_HIP(hipMemcpyAsync(sb.data(), d_sb.p, sb.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  VILO_HIP(hipMemcpyAsync(ex.data(), d_ex.p, ex.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  VILO_HIP(hipStreamSynchronize(ctx->stream));
  for (int w = 0; w < W; ++w) {
    memcpy(after[w].pose, &pose[(size_t)w * F * 7], sizeof(double) * F * 7);
    memcpy(after[w].speed_bias, &sb[(size_t)w * F * 9], sizeof(double) * F * 9);
    memcpy(after[w].ex_pose, &ex[(size_t)w * 14], sizeof(double) * 14);
  }
  return VILO_OK;
}
