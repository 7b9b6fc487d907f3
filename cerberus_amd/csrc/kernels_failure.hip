// Estimator::failureDetection (estimator.cpp:1005-1052) of every window of a resident batch, at its device state
// (vilo_batch_failure_detection, include/vilo_gpu.h). The reference's function returns false on its first line; every criterion of the text
// below that line is evaluated here, literally, as a flag bit.
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_failure_detection  lane = window, 64 windows per workgroup. A window reads the last frame's pose (7) and biases (6) and the caller's
//                        last pose (7) and track count; about 120 FP64 operations, two square roots of norms, one acos. Nothing crosses
//                        lanes: no LDS, no atomics. The six compared quantities go out as three 16-byte stores (48-byte rows of a
//                        256-byte aligned block).
//
// Floating-point contraction is off for the whole file, the inlined helpers of vilo_math.hpp included: the numpy definition
// (tests/gauge_ref.py) rounds every operation, and a flag must not depend on a fused multiply-add the reference's compiler did not make.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_window_failure_record) == 12, "vilo_window_failure_record: 12 bytes (include/vilo_gpu.h)");

#define FD_THREADS 64
#define FD_VALUES 6

struct FailureArgs {
  const int *last_track_num;           // [W], or null
  const double *last_pose;             // [W][7], or null
  vilo_window_failure_record *rec;     // [W]
  double *values;                      // [W][FD_VALUES]
};

namespace {
__device__ __forceinline__ bool fd_finite3(const vilo::v3 &v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
__device__ __forceinline__ bool fd_finiteq(const vilo::quat &q) { return isfinite(q.w) && isfinite(q.x) && isfinite(q.y) && isfinite(q.z); }
}  // namespace

__global__ void __launch_bounds__(FD_THREADS) k_failure_detection(BatchDev b, FailureArgs a) {
  using namespace vilo;
  const int win = blockIdx.x * FD_THREADS + threadIdx.x;
  if (win >= b.W) return;
  const int n = b.win[win].n_frames - 1;   // (a packed window has at least one frame)
  const double *x = b.x + (size_t)win * XSTRIDE;
  const double *pose = x + XO_POSE + 7 * n, *sb = x + XO_SB + 9 * n;
  const v3 Ba = ld3(sb + 3), Bg = ld3(sb + 6);
  bool finite = fd_finite3(Ba) && fd_finite3(Bg);
  int flags = 0;
  double val[FD_VALUES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // the compared quantities, in bit order (constant indices: registers)
  // :1008
  if (a.last_track_num) {
    const int tracks = a.last_track_num[win];
    val[0] = (double)tracks;
    if (tracks < 2) flags |= VILO_FAILURE_FEW_TRACKS;
  }
  // :1013, :1018
  val[1] = norm(Ba);
  val[2] = norm(Bg);
  if (val[1] > 2.5) flags |= VILO_FAILURE_BIG_BA;
  if (val[2] > 1.0) flags |= VILO_FAILURE_BIG_BG;
  if (a.last_pose) {
    const double *lp = a.last_pose + 7 * (size_t)win;
    const v3 P = ld3(pose), last_P = ld3(lp);
    const quat q = ldq_pose(pose), last_q = ldq_pose(lp);
    finite = finite && fd_finite3(P) && fd_finite3(last_P) && fd_finiteq(q) && fd_finiteq(last_q);
    // :1030-1040
    val[3] = norm(P - last_P);
    if (val[3] > 5) flags |= VILO_FAILURE_BIG_TRANSLATION;
    val[4] = fabs(P.z - last_P.z);
    if (val[4] > 1) flags |= VILO_FAILURE_BIG_Z;
    // :1041-1046 (3.14 is the reference's; a NaN from an argument above 1 compares false)
    const m3 delta_R = tr(qR(qnormalized(q))) * qR(qnormalized(last_q));
    const quat delta_Q = quat_from_R_dev(delta_R);
    val[5] = acos(delta_Q.w) * 2.0 / 3.14 * 180.0;
    if (val[5] > 50) flags |= VILO_FAILURE_BIG_ANGLE;
  }
  vilo_window_failure_record r;
  r.status = finite ? VILO_FAILURE_OK : VILO_FAILURE_NUMERIC;
  if (!finite) {
    flags = 0;
    for (int k = 0; k < FD_VALUES; ++k) val[k] = 0.0;
  }
  r.flags = flags;
  r.would_reboot = (flags & (VILO_FAILURE_BIG_BA | VILO_FAILURE_BIG_BG)) ? 1 : 0;
  a.rec[win] = r;
  double2 *out = (double2 *)(a.values + (size_t)FD_VALUES * win);
  out[0] = make_double2(val[0], val[1]); out[1] = make_double2(val[2], val[3]); out[2] = make_double2(val[4], val[5]);
}

extern "C" int vilo_batch_failure_detection(vilo_ctx *ctx, vilo_batch *bt, const int32_t *last_track_num, const double *last_pose,
                                            vilo_window_failure_record *records, double *values_out) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (W > 0 && !records) {
    ctx->err = "vilo_batch_failure_detection: records is NULL";
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_failure_ms);
  if (W == 0) return VILO_OK;
  // the call's device memory: track counts | last poses | records | values
  const size_t o_t = call.lay.take<int32_t>(W, last_track_num != nullptr), o_p = call.lay.take<double>(7 * (size_t)W, last_pose != nullptr);
  const size_t o_r = call.lay.take<vilo_window_failure_record>(W), o_v = call.lay.take<double>(FD_VALUES * (size_t)W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  FailureArgs a;
  a.last_track_num = last_track_num ? call.ptr<int>(o_t) : nullptr;
  a.last_pose = last_pose ? call.ptr<double>(o_p) : nullptr;
  a.rec = call.ptr<vilo_window_failure_record>(o_r);
  a.values = call.ptr<double>(o_v);
  // (not timed)
  if (last_track_num) VILO_HIP(hipMemcpyAsync(call.ptr<int>(o_t), last_track_num, sizeof(int32_t) * (size_t)W, hipMemcpyHostToDevice, ctx->stream));
  if (last_pose) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_p), last_pose, sizeof(double) * 7 * (size_t)W, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_failure_detection, dim3((W + FD_THREADS - 1) / FD_THREADS), dim3(FD_THREADS), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_failure_record) * (size_t)W));
  VILO_HIP(call.down(values_out, a.values, sizeof(double) * FD_VALUES * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_failure_detection(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                             const int32_t *last_track_num, const double *last_pose, vilo_window_failure_record *records,
                                             double *values_out) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  if (!records) {
    ctx->err = "vilo_window_failure_detection: records is NULL";
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state,
                         [&](vilo_batch *bt) { return vilo_batch_failure_detection(ctx, bt, last_track_num, last_pose, records, values_out); });
}

extern "C" double vilo_last_failure_detection_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_failure_ms : -1.0; }
