// Mid-point dead reckoning of a frame's state through IMU samples (vilo_batch_dead_reckon, include/vilo_gpu.h; Estimator::processIMULeg,
// estimator.cpp:639-646, on the newest frame, which starts as a copy of the one before it, :794-802; fastPredictIMU / updateLatestStates,
// :1800-1840, the same recurrence after every image).
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_dead_reckon  lane = window, 64 windows per workgroup. The recurrence is a chain: every step needs the R, P, V of the step before,
//                  about 110 FP64 operations of which the 3 x 3 product R * R(deltaQ) and the two R * v are the bulk, so a window is
//                  one lane's work and the batch supplies the parallelism; nothing crosses lanes, no LDS, no atomics. P, V, R (15 values)
//                  and the biases stay in registers for the whole range. The host has packed every sample to the seven doubles a step
//                  reads (dt acc gyr: DR_ROW, 56 of vilo_sample's 280 bytes), so a lane streams its window's contiguous rows: 56-byte
//                  rows are 8-byte aligned, hence seven 8-byte loads (lanes of a wave read rows a window's range apart: what a wave
//                  fetches is 64 short streams, each of them sequential). The loads of row i + 1 are issued at the top of step i,
//                  ahead of the dependent chain, and first used at step i + 1 (the producer loop of kernels_preint.hip keeps its
//                  samples one step ahead the same way). With a trajectory asked for, every step writes its state row as five 16-byte stores (80-byte rows of a
//                  256-byte aligned block: 16-byte aligned).
//
// The quaternion of a state row is Eigen's Quaterniond(Matrix3d) of R as it stands (vilo_math.hpp's quat_from_R_dev): neither R nor the quaternion is normalised between
// steps or at the end, as the reference's Rs[j] is not. Floating-point contraction is off for the whole file, the inlined helpers of
// vilo_math.hpp included: a trajectory's last row and state_out are the same function of the same values and must be the same bits,
// and the numpy definition (tests/deadreckon_ref.py) rounds every operation.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "deadreckon_host.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_dead_reckon_opts) == 8, "vilo_dead_reckon_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_dead_reckon_record) == 8, "vilo_window_dead_reckon_record: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_sample) == 8 * 35, "vilo_sample: 35 doubles (include/vilo_gpu.h)");

#define DR_THREADS 64

struct DeadReckonArgs {
  int from_frame, write;
  double g_norm;
  const double *rows;           // [n_samples][DR_ROW] packed samples
  const int *offsets;           // [W + 1] window w reads rows offsets[w] .. offsets[w + 1]
  const int *step_offsets;      // [W + 1] window w's trajectory rows
  double *state;                // [W][DR_STATE]
  double *traj;                 // [sum n_steps][DR_STATE], or null
  vilo_window_dead_reckon_record *rec;   // [W]
};

namespace {

struct DrRow { double2 a, b, c, d, e; };   // P.x P.y | P.z q.x | q.y q.z | q.w V.x | V.y V.z

__device__ __forceinline__ DrRow dr_row(const vilo::v3 &P, const vilo::m3 &R, const vilo::v3 &V) {
  const vilo::quat q = vilo::quat_from_R_dev(R);
  DrRow r;
  r.a = make_double2(P.x, P.y); r.b = make_double2(P.z, q.x); r.c = make_double2(q.y, q.z);
  r.d = make_double2(q.w, V.x); r.e = make_double2(V.y, V.z);
  return r;
}
__device__ __forceinline__ void dr_store(double *dst, const DrRow &r) {
  double2 *p = (double2 *)dst;
  p[0] = r.a; p[1] = r.b; p[2] = r.c; p[3] = r.d; p[4] = r.e;
}
__device__ __forceinline__ bool dr_finite3(const vilo::v3 &v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

}  // namespace

__global__ void __launch_bounds__(DR_THREADS) k_dead_reckon(BatchDev b, DeadReckonArgs a) {
  using namespace vilo;
  const int win = blockIdx.x * DR_THREADS + threadIdx.x;
  if (win >= b.W) return;
  const int n_frames = b.win[win].n_frames;
  const int f = a.from_frame < 0 ? n_frames - 1 : a.from_frame;
  const int s_begin = a.offsets[win], n = a.offsets[win + 1] - s_begin;
  const int n_steps = n > 1 ? n - 1 : 0;
  double *traj = a.traj ? a.traj + (size_t)DR_STATE * a.step_offsets[win] : nullptr;
  double *x = b.x + (size_t)win * XSTRIDE;

  // (the range, the status and the record are written out here, not taken from SampleRange: DESIGN 4.36)
  int status = VILO_DR_OK;
  DrRow out;
  out.a = out.b = out.c = out.d = out.e = make_double2(0.0, 0.0);
  // (f <= VILO_MAX_FRAMES - 1 by the argument check and n_frames <= VILO_MAX_FRAMES: rows f and, with write, f + 1 of the state exist)
  if (f < 0 || f >= n_frames || (a.write && f + 1 >= n_frames)) status = VILO_DR_NO_FRAME;
  else {
    const double *pose = x + XO_POSE + 7 * f, *sb = x + XO_SB + 9 * f;
    v3 P = ld3(pose), V = ld3(sb);
    const v3 ba = ld3(sb + 3), bg = ld3(sb + 6);
    const quat q0 = ldq_pose(pose);
    bool finite = dr_finite3(P) && dr_finite3(V) && dr_finite3(ba) && dr_finite3(bg) && isfinite(q0.w) && isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z);
    m3 R = qR(qnormalized(q0));
    const v3 g = mk3(0.0, 0.0, a.g_norm);
    if (n_steps > 0) {
      const double *row = a.rows + (size_t)DR_ROW * s_begin;
      // the first sample of the range: (acc_0, gyr_0); its dt is not read
      v3 acc_0 = ld3(row + 1), gyr_0 = ld3(row + 4);
      finite = finite && dr_finite3(acc_0) && dr_finite3(gyr_0);
      double nxt[DR_ROW];
#pragma unroll
      for (int k = 0; k < DR_ROW; ++k) nxt[k] = row[DR_ROW + k];
      for (int i = 1; i < n; ++i) {
        double cur[DR_ROW];
#pragma unroll
        for (int k = 0; k < DR_ROW; ++k) cur[k] = nxt[k];
        if (i + 1 < n) {
          // row i + 1, in flight over this step's chain
          const double *nr = row + (size_t)DR_ROW * (i + 1);
#pragma unroll
          for (int k = 0; k < DR_ROW; ++k) nxt[k] = nr[k];
        }
        const double dt = cur[0];
        const v3 acc_1 = ld3(cur + 1), gyr_1 = ld3(cur + 4);
        finite = finite && isfinite(dt) && dr_finite3(acc_1) && dr_finite3(gyr_1);
        // estimator.cpp:640-646
        const v3 un_acc_0 = R * (acc_0 - ba) - g;
        const v3 un_gyr = (gyr_0 + gyr_1) * 0.5 - bg;
        R = R * qR(deltaQ(un_gyr * dt));
        const v3 un_acc_1 = R * (acc_1 - ba) - g;
        const v3 un_acc = (un_acc_0 + un_acc_1) * 0.5;
        P = P + (V * dt + un_acc * (0.5 * dt * dt));
        V = V + un_acc * dt;
        acc_0 = acc_1; gyr_0 = gyr_1;
        if (traj) dr_store(traj + (size_t)DR_STATE * (i - 1), dr_row(P, R, V));
      }
    }
    out = dr_row(P, R, V);
    finite = finite && isfinite(out.a.x) && isfinite(out.a.y) && isfinite(out.b.x) && isfinite(out.b.y) && isfinite(out.c.x) && isfinite(out.c.y) &&
             isfinite(out.d.x) && isfinite(out.d.y) && isfinite(out.e.x) && isfinite(out.e.y);
    if (!finite) status = VILO_DR_NUMERIC;
  }
  if (status != VILO_DR_OK) {
    out.a = out.b = out.c = out.d = out.e = make_double2(0.0, 0.0);
    if (traj)
      for (int i = 0; i < n_steps; ++i) dr_store(traj + (size_t)DR_STATE * i, out);
  } else if (a.write) {
    // frame f + 1's pose row [P, q as x y z w] and velocity; its biases and leg biases stay
    double *pose = x + XO_POSE + 7 * (f + 1), *sb = x + XO_SB + 9 * (f + 1);
    pose[0] = out.a.x; pose[1] = out.a.y; pose[2] = out.b.x; pose[3] = out.b.y; pose[4] = out.c.x; pose[5] = out.c.y; pose[6] = out.d.x;
    sb[0] = out.d.y; sb[1] = out.e.x; sb[2] = out.e.y;
  }
  dr_store(a.state + (size_t)DR_STATE * win, out);
  vilo_window_dead_reckon_record r;
  r.n_steps = n_steps;
  r.status = status;
  a.rec[win] = r;
}

extern "C" void vilo_default_dead_reckon_opts(vilo_dead_reckon_opts *o) {
  if (!o) return;
  o->from_frame = -1;
  o->write = 0;
}

static const char DEAD_RECKON_CALL[] = "vilo_batch_dead_reckon";

extern "C" int vilo_batch_dead_reckon(vilo_ctx *ctx, vilo_batch *bt, const vilo_dead_reckon_opts *opts, const vilo_sample *samples,
                                      const int32_t *offsets, double *state_out, double *trajectory_out, vilo_window_dead_reckon_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  const vilo_dead_reckon_opts o = sample_call_opts(opts, vilo_default_dead_reckon_opts);
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (const char *what = vilo::dead_reckon_check(o, W, samples, offsets, state_out)) return sample_call_fail(ctx, DEAD_RECKON_CALL, what, VILO_ERR_BAD_ARG);
  BatchCall call(ctx, bt, &vilo_ctx::last_dead_reckon_ms);
  if (W == 0) return VILO_OK;
  SampleUpload up(ctx, call, DEAD_RECKON_CALL, W, samples, offsets, DR_ROW, vilo::dead_reckon_pack);
  if (!up.staged()) return VILO_ERR_HIP;
  const size_t n_rows = (size_t)up.n_rows;
  const bool want_traj = trajectory_out != nullptr;
  // the call's device memory after the samples': states | trajectory | records
  const size_t o_x = call.lay.take<double>(DR_STATE * (size_t)W), o_j = call.lay.take<double>(DR_STATE * n_rows, want_traj);
  const size_t o_c = call.lay.take<vilo_window_dead_reckon_record>(W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(up.send(call));
  DeadReckonArgs a;
  a.from_frame = o.from_frame; a.write = o.write;
  a.g_norm = ctx->cfg.g_norm;
  a.rows = up.rows;
  a.offsets = up.offsets;
  a.step_offsets = up.step_offsets;
  a.state = call.ptr<double>(o_x);
  a.traj = want_traj && n_rows > 0 ? call.ptr<double>(o_j) : nullptr;
  a.rec = call.ptr<vilo_window_dead_reckon_record>(o_c);
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_dead_reckon, dim3((W + DR_THREADS - 1) / DR_THREADS), dim3(DR_THREADS), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(state_out, a.state, sizeof(double) * DR_STATE * (size_t)W));
  if (want_traj) VILO_HIP(call.down(trajectory_out, a.traj, sizeof(double) * DR_STATE * n_rows));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_dead_reckon_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_dead_reckon(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                                       const vilo_dead_reckon_opts *opts, const vilo_sample *samples, const int32_t *offsets, double *state_out,
                                       double *trajectory_out, vilo_window_dead_reckon_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  const vilo_dead_reckon_opts o = sample_call_opts(opts, vilo_default_dead_reckon_opts);
  if (const char *what = vilo::dead_reckon_check(o, n_windows, samples, offsets, state_out)) return sample_call_fail(ctx, DEAD_RECKON_CALL, what, VILO_ERR_BAD_ARG);
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_dead_reckon(ctx, bt, &o, samples, offsets, state_out, trajectory_out, records);
    if (r != VILO_OK || !o.write) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);   // (the other state arrays come back as they went up)
  });
}

extern "C" double vilo_last_dead_reckon_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_dead_reckon_ms : -1.0; }
