// Gyroscope-bias alignment of a batch's windows (vilo_batch_gyro_bias_align, include/vilo_gpu.h; solveGyroscopeBias,
// src/initial/initial_aligment.cpp:14-40, without the trailing repropagate loop).
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_gyro_bias_align  16 lanes per window, lane = interval (at most 10 live), four windows per wave, 16 per 256-thread workgroup. The work
//                      is a handful of flops per interval; what costs is the latency of the few cache lines a lane needs out of its
//                      interval's 15.6 KB record (delta_q, lin_bg, three rows of the Jacobian block) and of two pose rows, so the mapping
//                      spreads the intervals over lanes to have all of a window's loads in flight at once. A lane forms its interval's
//                      6 + 3 + 1 terms of A = sum J^T J, b = sum J^T r, sum |r|^2; a dead lane contributes zeros. An xor butterfly over
//                      offsets 8, 4, 2, 1 leaves every lane of the 16 with the same bits (both partners add the same two values): no
//                      atomics, no LDS. Every lane does the unpivoted 3 x 3 LDL^T redundantly, so the status tests are uniform over the 16;
//                      a second butterfly gives the model cost. Lane 0 writes delta_bg and the record; with `write`, lane f < n_frames
//                      adds delta_bg to frame f's gyro bias of the batch's current state (the lane that read Bg_f is the lane that
//                      writes it).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>

#include "batch_call.hpp"
#include "lin_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_gyro_opts) == 8, "vilo_gyro_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_gyro_record) == 24, "vilo_window_gyro_record: 24 bytes (include/vilo_gpu.h)");

#define GYRO_THREADS 256
#define GYRO_LANES 16      // lanes of a window: one per interval, VILO_MAX_FRAMES - 1 = 10 of them live at most
#define GYRO_NSUM 10       // upper triangle of A (6), b (3), sum |r|^2

// where an interval's record keeps what the alignment reads, in doubles from the start of the record array
struct GyroRecLayout {
  const double *rec;   // [W * 10] vilo_preint or vilo_preint_imu
  int stride;          // doubles per record
  int o_dq, o_bg;      // delta_q [x y z w], lin_bg
  int o_jac, ld;       // entry (O_R, O_BG) of the row-major Jacobian and its row length: (3, 24) of 31 x 31, (3, 12) of 15 x 15
};

struct GyroArgs {
  int corrected, write;
  double *delta_bg;                // [W][3]
  vilo_window_gyro_record *rec;    // [W]
};

__global__ void __launch_bounds__(GYRO_THREADS) k_gyro_bias_align(BatchDev b, GyroRecLayout L, GyroArgs a) {
  using namespace vilo;
  const int win = blockIdx.x * (GYRO_THREADS / GYRO_LANES) + (threadIdx.x / GYRO_LANES), k = threadIdx.x % GYRO_LANES;
  // (a window past the batch's end takes the last window's place and writes nothing: the shuffles below want every lane of the wave)
  const bool win_ok = win < b.W;
  const int wi = win_ok ? win : b.W - 1;
  const int n_frames = b.win[wi].n_frames;
  const int n_int = n_frames - 1;
  const bool live = k < n_int;   // (n_int <= VILO_MAX_FRAMES - 1 = 10: rows k and k + 1 of the state exist)
  double *x = b.x + (size_t)wi * XSTRIDE;

  m3 J = m3_zero();
  v3 r = mk3(0.0, 0.0, 0.0);
  if (live) {
    const double *p = L.rec + ((size_t)wi * 10 + k) * L.stride;
    const quat qi = qnormalized(ldq_pose(x + XO_POSE + 7 * k)), qj = qnormalized(ldq_pose(x + XO_POSE + 7 * (k + 1)));
    const double *jp = p + L.o_jac;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int c = 0; c < 3; ++c) J.a[3 * rr + c] = jp[rr * L.ld + c];
    }
    quat g = mkq(p[L.o_dq + 3], p[L.o_dq], p[L.o_dq + 1], p[L.o_dq + 2]);
    if (a.corrected) {
      // the corrected rotation of the IMU factors (factors.hpp, imu_leg_raw): delta_q (x) deltaQ(dq_dbg (Bg_k - lin_bg))
      const v3 dbg = ld3(x + XO_SB + 9 * k + 6) - ld3(p + L.o_bg);
      g = qmul(g, deltaQ(J * dbg));
    }
    // (the reference takes q_ij from R_k^T R_{k+1}, whose quaternion has w >= 0 whichever hemisphere the stored pose quaternions lie in:
    // the product is brought to w >= 0, which negates nothing while neighbouring poses share a hemisphere)
    const quat e = qmul(qinv(g), qmul(qinv(qi), qj));
    r = qvec(e) * (e.w < 0.0 ? -2.0 : 2.0);
  }
  double s[GYRO_NSUM];
  {
    int e = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = i; j < 3; ++j) s[e++] = J.a[i] * J.a[j] + J.a[3 + i] * J.a[3 + j] + J.a[6 + i] * J.a[6 + j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) s[6 + i] = J.a[i] * r.x + J.a[3 + i] * r.y + J.a[6 + i] * r.z;
    s[9] = dot(r, r);
  }
  lanes_sum<GYRO_NSUM, GYRO_LANES>(s);   // over the 16 lanes of a window

  int status = VILO_GYRO_OK;
  double d[3] = {0.0, 0.0, 0.0};
  bool finite = true;
#pragma unroll
  for (int i = 0; i < GYRO_NSUM; ++i) finite = finite && isfinite(s[i]);
  if (n_int < 1) status = VILO_GYRO_NO_INTERVALS;
  else if (!finite) status = VILO_GYRO_NUMERIC;
  else {
    // A = L D L^T without pivoting (A: s[0..5] = a00 a01 a02 a11 a12 a22), then L z = b, D y = z, L^T d = y. The pivots are tested in
    // order: the first that is not positive decides, and nothing is divided by it.
    auto bad = [&](double p) {
      if (p > 0.0) return false;
      status = isnan(p) ? VILO_GYRO_NUMERIC : VILO_GYRO_SINGULAR;
      return true;
    };
    const double d0 = s[0];
    if (!bad(d0)) {
      const double l10 = s[1] / d0, l20 = s[2] / d0;
      const double d1 = s[3] - l10 * s[1];
      if (!bad(d1)) {
        const double u12 = s[4] - l20 * s[1];
        const double l21 = u12 / d1;
        const double d2 = s[5] - l20 * s[2] - l21 * u12;
        if (!bad(d2)) {
          const double z0 = s[6], z1 = s[7] - l10 * z0, z2 = s[8] - l20 * z0 - l21 * z1;
          d[2] = z2 / d2;
          d[1] = z1 / d1 - l21 * d[2];
          d[0] = z0 / d0 - l10 * d[1] - l20 * d[2];
          if (!(isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]))) { status = VILO_GYRO_NUMERIC; d[0] = d[1] = d[2] = 0.0; }
        }
      }
    }
  }
  // model cost at the step (the initial cost's own sum when the step is zero)
  double mc[1];
  {
    const v3 e = r - J * mk3(d[0], d[1], d[2]);
    mc[0] = dot(e, e);
  }
  lanes_sum<1, GYRO_LANES>(mc);

  if (!win_ok) return;
  if (k == 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) a.delta_bg[(size_t)3 * win + i] = d[i];
    vilo_window_gyro_record o;
    o.initial_cost = 0.5 * s[9];
    o.model_cost = 0.5 * mc[0];
    o.n_intervals = n_int < 0 ? 0 : n_int;
    o.status = status;
    a.rec[win] = o;
  }
  if (a.write && status == VILO_GYRO_OK && k < n_frames) {
    double *bg = x + XO_SB + 9 * k + 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) bg[i] = bg[i] + d[i];
  }
}

extern "C" void vilo_default_gyro_opts(vilo_gyro_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->linearization = VILO_GYRO_RECORD;
  o->write = 0;
}

static int gyro_check_opts(vilo_ctx *ctx, const vilo_gyro_opts *opts, vilo_gyro_opts *o) {
  if (opts) *o = *opts; else vilo_default_gyro_opts(o);
  if (o->linearization != VILO_GYRO_RECORD && o->linearization != VILO_GYRO_CORRECTED) {
    ctx->err = "vilo_batch_gyro_bias_align: linearization must be VILO_GYRO_RECORD or VILO_GYRO_CORRECTED";
    return VILO_ERR_BAD_ARG;
  }
  if (o->write != 0 && o->write != 1) {
    ctx->err = "vilo_batch_gyro_bias_align: write must be 0 or 1";
    return VILO_ERR_BAD_ARG;
  }
  return VILO_OK;
}

extern "C" int vilo_batch_gyro_bias_align(vilo_ctx *ctx, vilo_batch *bt, const vilo_gyro_opts *opts, double *delta_bg, vilo_window_gyro_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_gyro_opts o;
  const int rc = gyro_check_opts(ctx, opts, &o);
  if (rc != VILO_OK) return rc;
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (W > 0 && !delta_bg) {
    ctx->err = "vilo_batch_gyro_bias_align: delta_bg is NULL";
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_gyro_ms);
  if (W == 0) return VILO_OK;
  const bool leg = bt->rec.leg;
  const void *recs = bt->rec.d_pre;
  if (!recs) {
    ctx->err = "vilo_batch_gyro_bias_align: the batch has no preintegration records";
    return VILO_ERR_UNSUPPORTED;
  }
  // the call's device memory: steps | records | re-integration copies. Only the integration: no factor is whitened here, so the sqrt_info
  // stage that follows it elsewhere is left out, and with it every write to the batch's prepared records and flags.
  const size_t o_d = call.lay.take<double>(3 * (size_t)W), o_r = call.lay.take<vilo_window_gyro_record>(W);
  const ReintegrationBlocks rp(call.lay, bd, 1);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(call.start());
  BatchDev b = bd;
  if (call.reintegrate(b, rp) != VILO_OK) return VILO_ERR_HIP;
  if (rp.on) recs = b.rp_pre;
  GyroRecLayout L;
  L.rec = (const double *)recs;
  if (leg) {
    L.stride = (int)(sizeof(vilo_preint) / sizeof(double));
    L.o_dq = (int)(offsetof(vilo_preint, delta_q) / sizeof(double)); L.o_bg = (int)(offsetof(vilo_preint, lin_bg) / sizeof(double));
    L.ld = VILO_RESIDUAL_STATE_SIZE; L.o_jac = (int)(offsetof(vilo_preint, jacobian) / sizeof(double)) + 3 * L.ld + 24;   // (ILO_R, ILO_BG)
  } else {
    L.stride = (int)(sizeof(vilo_preint_imu) / sizeof(double));
    L.o_dq = (int)(offsetof(vilo_preint_imu, delta_q) / sizeof(double)); L.o_bg = (int)(offsetof(vilo_preint_imu, lin_bg) / sizeof(double));
    L.ld = 15; L.o_jac = (int)(offsetof(vilo_preint_imu, jacobian) / sizeof(double)) + 3 * L.ld + 12;   // (O_R, O_BG)
  }
  GyroArgs a;
  a.corrected = o.linearization == VILO_GYRO_CORRECTED ? 1 : 0; a.write = o.write;
  a.delta_bg = call.ptr<double>(o_d);
  a.rec = call.ptr<vilo_window_gyro_record>(o_r);
  const int per_block = GYRO_THREADS / GYRO_LANES;
  hipLaunchKernelGGL(k_gyro_bias_align, dim3((W + per_block - 1) / per_block), dim3(GYRO_THREADS), 0, ctx->stream, bd, L, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(delta_bg, a.delta_bg, sizeof(double) * 3 * (size_t)W));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_gyro_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_gyro_bias_align(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state,
                                           const vilo_gyro_opts *opts, double *delta_bg, vilo_window_gyro_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_gyro_opts o;
  const int rc = gyro_check_opts(ctx, opts, &o);
  if (rc != VILO_OK) return rc;
  if (!delta_bg) {
    ctx->err = "vilo_window_gyro_bias_align: delta_bg is NULL";
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_gyro_bias_align(ctx, bt, &o, delta_bg, records);
    if (r != VILO_OK || !o.write) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);   // (the other state arrays come back as they went up)
  });
}

extern "C" double vilo_last_gyro_align_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_gyro_ms : -1.0; }
