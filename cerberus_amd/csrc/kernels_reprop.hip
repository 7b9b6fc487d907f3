// The preintegration records of a resident batch integrated again ONCE, at chosen biases (vilo_batch_repropagate, include/vilo_gpu.h):
// the reference's start-up loop `il_pre_integrations[i]->repropagate(Vector3d::Zero(), Bgs[i], Rhos[i])` (estimator.cpp:752-760) and the
// loop at the end of solveGyroscopeBias (initial_aligment.cpp:42-47), after which the solve runs on fixed records.
//
// One code path for every batch size (no launch plan, no switch; no output of an interval depends on the batch it shares, nor on its
// position):
//   k_reprop_point   lane = interval, 64 intervals per workgroup. An interval reads its state rows (6 + 4 doubles), the record's own
//                    lin_ba / lin_bg / lin_rho (10 consecutive doubles) and, by mode, the caller's row or mask byte; forms the point, the
//                    three drifts, `selected` and the status, and writes the row the integrator takes, the "integrate" flag and the
//                    preparation's skip byte. Nothing crosses lanes: no LDS, no atomics. The record goes out as two 16-byte stores.
//   (integration)    k_preint_imu_leg / k_preint_imu of kernels_preint.hip, the kernels behind vilo_preintegrate, over the uploaded
//                    samples with that row, into records of the call's own memory; an interval whose flag is 0 returns at once.
//   k_reprop_commit  one wave per record: the flagged records into the batch's array with 16-byte loads and stores (a record is an odd
//                    number of doubles, so every second one starts 8 bytes off a 16-byte boundary: one 8-byte access at that end), and
//                    the cleared "no sqrt_info" flag the preparation sets again. Used a second time for the prepared form of IMU-only
//                    records, which is built on copies (k_embed_sqrt15 rewrites in place and must not see a record twice).
//   (preparation)    k_prepare_preint / k_prepare_preint_imu of kernels_eval.hip on the flagged records only.
//
// Floating-point contraction is off for the whole file: the numpy definition (tests/reprop_ref.py) rounds every operation, and a
// selection must not depend on a fused multiply-add.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include <cmath>
#include <vector>

#include "batch_call.hpp"

static_assert(sizeof(vilo_interval_reprop_record) == 32, "vilo_interval_reprop_record: 32 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_reprop_opts) == 40, "vilo_reprop_opts: 40 bytes (include/vilo_gpu.h)");
static_assert(offsetof(vilo_preint, lin_bg) == offsetof(vilo_preint, lin_ba) + 24 && offsetof(vilo_preint, lin_rho) == offsetof(vilo_preint, lin_ba) + 48,
              "lin_ba(3) lin_bg(3) lin_rho(4) are consecutive in vilo_preint");
static_assert(offsetof(vilo_preint_imu, lin_bg) == offsetof(vilo_preint_imu, lin_ba) + 24, "lin_ba(3) lin_bg(3) are consecutive in vilo_preint_imu");

#define RP_THREADS 64

struct RepropArgs {
  int point, select, write, leg;
  double th_ba, th_bg, th_rho;
  const double *rec;                   // the batch's records as doubles
  int stride, o_lin;                   // doubles per record, offset of lin_ba in it
  const double *lin_in;                // [NF][10], POINT_GIVEN
  const unsigned char *mask;           // [NF], SELECT_MASK
  const int *offsets;                  // [NF + 1], or null (write == 0)
  double *lin_out;                     // [NF][10 or 6]: the integrator's rows
  vilo_interval_reprop_record *out;    // [NF]
  int *go;                             // [NF] 1: integrate and commit this interval
  unsigned char *prep_skip;            // [NF] 0: prepare this record again
};

__global__ void __launch_bounds__(RP_THREADS) k_reprop_point(BatchDev b, RepropArgs a) {
  const int f = blockIdx.x * RP_THREADS + threadIdx.x;
  if (f >= b.W * 10) return;
  const int win = f / 10, k = f - 10 * win;
  const int nl = a.leg ? 10 : 6;
  double p[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double dr[3] = {0.0, 0.0, 0.0};
  int selected = 0, status = VILO_REPROP_NO_INTERVAL;
  if (k < b.win[win].n_frames - 1) {
    const double *x = b.x + (size_t)win * XSTRIDE;
    if (a.point == VILO_REPROP_POINT_GIVEN) {
      for (int i = 0; i < 10; ++i) p[i] = i < nl ? a.lin_in[(size_t)10 * f + i] : 0.0;
    } else {
      const int fr = a.point == VILO_REPROP_POINT_STARTUP ? k + 1 : k;
      const double *sb = x + XO_SB + 9 * fr, *lb = x + XO_LB + 4 * fr;
      for (int i = 0; i < 3; ++i) { p[i] = a.point == VILO_REPROP_POINT_STARTUP ? 0.0 : sb[3 + i]; p[3 + i] = sb[6 + i]; }
      for (int i = 0; i < 4; ++i) p[6 + i] = a.leg ? lb[i] : 0.0;
    }
    bool finite = true;
    for (int i = 0; i < 10; ++i) finite = finite && isfinite(p[i]);
    if (!finite) {
      status = VILO_REPROP_NUMERIC;
    } else {
      const double *rl = a.rec + (size_t)a.stride * f + a.o_lin;
      double d[10];
      for (int i = 0; i < 10; ++i) d[i] = i < nl ? p[i] - rl[i] : 0.0;
      dr[0] = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      dr[1] = sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5]);
      dr[2] = sqrt(((d[6] * d[6] + d[7] * d[7]) + d[8] * d[8]) + d[9] * d[9]);
      if (a.select == VILO_REPROP_SELECT_ALL) selected = 1;
      else if (a.select == VILO_REPROP_SELECT_MASK) selected = a.mask[f] != 0 ? 1 : 0;
      else selected = (dr[0] <= a.th_ba && dr[1] <= a.th_bg && dr[2] <= a.th_rho) ? 0 : 1;   // (a drift that is no number selects)
      status = !selected ? VILO_REPROP_NOT_SELECTED
               : (a.write && a.offsets[f + 1] - a.offsets[f] < 2) ? VILO_REPROP_NO_SAMPLES : VILO_REPROP_OK;
    }
  }
  const int go = (a.write && selected && status == VILO_REPROP_OK) ? 1 : 0;
  a.go[f] = go;
  a.prep_skip[f] = (go && !b.imu_skip[f]) ? 0 : 1;
  for (int i = 0; i < 10; ++i)
    if (i < nl) a.lin_out[(size_t)nl * f + i] = p[i];
  double2 *o = (double2 *)(a.out + f);   // (32-byte records of a 256-byte aligned block)
  o[0] = make_double2(dr[0], dr[1]);
  o[1] = make_double2(dr[2], __hiloint2double(status, selected));
}

// record f of src over record f of dst where go[f]; n_dbl doubles per record, both arrays 16-byte aligned at record 0
__global__ void __launch_bounds__(RP_THREADS) k_reprop_commit(int n, int n_dbl, const double *src, double *dst, const int *go, int *clear_flag) {
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f >= n || !go[f]) return;
  const size_t first = (size_t)f * n_dbl;
  const int head = (int)(first & 1), pairs = (n_dbl - head) >> 1, tail = (n_dbl - head) & 1;
  const double *s = src + first;
  double *d = dst + first;
  if (lane == 0 && head) d[0] = s[0];
  const double2 *s2 = (const double2 *)(s + head);
  double2 *d2 = (double2 *)(d + head);
  for (int e = lane; e < pairs; e += RP_THREADS) d2[e] = s2[e];
  if (lane == 0 && tail) d[n_dbl - 1] = s[n_dbl - 1];
  if (lane == 0 && clear_flag) clear_flag[f] = 0;
}

extern "C" void vilo_default_reprop_opts(vilo_reprop_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->point = VILO_REPROP_POINT_STATE;
  o->select = VILO_REPROP_SELECT_ALL;
  o->write = 1;
  o->ba_threshold = 0.10; o->bg_threshold = 0.01; o->rho_threshold = 0.01;
}

static int reprop_check_opts(vilo_ctx *ctx, const vilo_reprop_opts *opts, const vilo_sample *samples, const int32_t *offsets, const double *lin,
                             const uint8_t *mask, vilo_reprop_opts *o) {
  if (opts) *o = *opts; else vilo_default_reprop_opts(o);
  const char *why = nullptr;
  if (o->point < VILO_REPROP_POINT_STATE || o->point > VILO_REPROP_POINT_GIVEN) why = "vilo_batch_repropagate: point must be VILO_REPROP_POINT_STATE, _STARTUP or _GIVEN";
  else if (o->select < VILO_REPROP_SELECT_ALL || o->select > VILO_REPROP_SELECT_MASK) why = "vilo_batch_repropagate: select must be VILO_REPROP_SELECT_ALL, _DRIFTED or _MASK";
  else if (o->write != 0 && o->write != 1) why = "vilo_batch_repropagate: write must be 0 or 1";
  else if (o->point == VILO_REPROP_POINT_GIVEN && !lin) why = "vilo_batch_repropagate: VILO_REPROP_POINT_GIVEN needs lin";
  else if (o->select == VILO_REPROP_SELECT_MASK && !mask) why = "vilo_batch_repropagate: VILO_REPROP_SELECT_MASK needs mask";
  else if (o->write && (!samples || !offsets)) why = "vilo_batch_repropagate: write needs samples and offsets";
  else if (!(o->ba_threshold >= 0.0 && o->bg_threshold >= 0.0 && o->rho_threshold >= 0.0) || !std::isfinite(o->ba_threshold) || !std::isfinite(o->bg_threshold) ||
           !std::isfinite(o->rho_threshold)) why = "vilo_batch_repropagate: a threshold is negative or not finite";
  if (!why) return VILO_OK;
  ctx->err = why;
  return VILO_ERR_BAD_ARG;
}

extern "C" int vilo_batch_repropagate(vilo_ctx *ctx, vilo_batch *bt, const vilo_sample *samples, const int32_t *offsets, const vilo_reprop_opts *opts,
                                      const double *lin, const uint8_t *mask, vilo_interval_reprop_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_reprop_opts o;
  int rc = reprop_check_opts(ctx, opts, samples, offsets, lin, mask, &o);
  if (rc != VILO_OK) return rc;
  BatchDev &bd = bt->d;
  const int W = bd.W;
  const size_t NF = (size_t)W * 10;
  if (offsets) {
    bool bad = offsets[0] < 0;
    for (size_t f = 0; f < NF && !bad; ++f) bad = offsets[f + 1] < offsets[f];
    if (bad) {
      ctx->err = "vilo_batch_repropagate: offsets must not be negative and must not decrease";
      return VILO_ERR_BAD_ARG;
    }
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_reprop_ms);
  if (W == 0) return VILO_OK;
  BatchRecords &R = bt->rec;
  if (!R.d_pre) {
    ctx->err = "vilo_batch_repropagate: the batch has no preintegration records on the device";
    return VILO_ERR_UNSUPPORTED;
  }
  if (R.from_pool) {
    ctx->err = "vilo_batch_repropagate: the batch's records were gathered from a vilo_preint_streams pool, whose objects own them";
    return VILO_ERR_UNSUPPORTED;
  }
  if (bd.rp_on) {
    ctx->err = "vilo_batch_repropagate: vilo_batch_set_samples is in force, the solve integrates every interval again at every point anyway (switch it off first)";
    return VILO_ERR_UNSUPPORTED;
  }
  const bool wr = o.write != 0, leg = R.leg;
  const int nl = leg ? 10 : 6;
  const size_t rec_bytes = leg ? sizeof(vilo_preint) : sizeof(vilo_preint_imu), rec_dbl = rec_bytes / sizeof(double);
  const size_t ns = wr ? (size_t)offsets[NF] : 0, tps = vilo_preint_terms_per_sample(R.leg);
  // the call's device memory: samples | offsets | caller's rows | mask | integrator's rows | records | flags | skip bytes | the
  // integrated records | the integrator's leg terms | (IMU-only) the prepared form before it is committed
  const size_t o_s = call.lay.take<vilo_sample>(ns, wr), o_o = call.lay.take<int32_t>(NF + 1, offsets != nullptr);
  const size_t o_li = call.lay.take<double>(10 * NF, o.point == VILO_REPROP_POINT_GIVEN), o_m = call.lay.take<uint8_t>(NF, o.select == VILO_REPROP_SELECT_MASK);
  const size_t o_lo = call.lay.take<double>(nl * NF), o_r = call.lay.take<vilo_interval_reprop_record>(NF), o_g = call.lay.take<int>(NF), o_k = call.lay.take<uint8_t>(NF);
  const size_t o_pre = call.lay.take<char>(rec_bytes * NF, wr), o_t = call.lay.take<double>(tps * ns, wr && tps > 0), o_pp = call.lay.take<PreintPrepared>(NF, wr && !leg);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  RepropArgs a;
  a.point = o.point; a.select = o.select; a.write = o.write; a.leg = R.leg;
  a.th_ba = o.ba_threshold; a.th_bg = o.bg_threshold; a.th_rho = o.rho_threshold;
  a.rec = (const double *)R.d_pre; a.stride = (int)rec_dbl;
  a.o_lin = (int)((leg ? offsetof(vilo_preint, lin_ba) : offsetof(vilo_preint_imu, lin_ba)) / sizeof(double));
  a.lin_in = o.point == VILO_REPROP_POINT_GIVEN ? call.ptr<double>(o_li) : nullptr;
  a.mask = o.select == VILO_REPROP_SELECT_MASK ? call.ptr<unsigned char>(o_m) : nullptr;
  a.offsets = offsets ? call.ptr<int>(o_o) : nullptr;
  a.lin_out = call.ptr<double>(o_lo); a.out = call.ptr<vilo_interval_reprop_record>(o_r); a.go = call.ptr<int>(o_g); a.prep_skip = call.ptr<unsigned char>(o_k);
  // (not timed)
  if (wr && ns) VILO_HIP(hipMemcpyAsync(call.ptr<vilo_sample>(o_s), samples, sizeof(vilo_sample) * ns, hipMemcpyHostToDevice, ctx->stream));
  if (offsets) VILO_HIP(hipMemcpyAsync(call.ptr<int>(o_o), offsets, sizeof(int32_t) * (NF + 1), hipMemcpyHostToDevice, ctx->stream));
  if (a.lin_in) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_li), lin, sizeof(double) * 10 * NF, hipMemcpyHostToDevice, ctx->stream));
  if (a.mask) VILO_HIP(hipMemcpyAsync(call.ptr<unsigned char>(o_m), mask, NF, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_reprop_point, dim3((unsigned)((NF + RP_THREADS - 1) / RP_THREADS)), dim3(RP_THREADS), 0, ctx->stream, bd, a);
  if (wr) {
    if (vilo_launch_preintegrate(ctx, R.leg, (int)NF, call.ptr<vilo_sample>(o_s), a.offsets, a.lin_out, call.ptr<char>(o_pre), tps ? call.ptr<double>(o_t) : nullptr,
                                 a.go) != VILO_OK) return VILO_ERR_HIP;
    hipLaunchKernelGGL(k_reprop_commit, dim3((unsigned)NF), dim3(RP_THREADS), 0, ctx->stream, (int)NF, (int)rec_dbl, (const double *)call.ptr<char>(o_pre), (double *)R.d_pre,
                       (const int *)a.go, bd.prep_bad);
    if (leg) {
      if (vilo_launch_prepare_preint(ctx, (int)NF, (const vilo_preint *)R.d_pre, bd.prep, bd.prep_bad, a.prep_skip, 1) != VILO_OK) return VILO_ERR_HIP;
    } else {
      // the 15 x 15 sqrt_info is embedded into the 31 x 31 the factor kernels read by a kernel that rewrites every record of its batch in
      // place: on copies (cleared: it reads the ones the preparation skipped too), of which the flagged ones are committed
      BatchDev bs = bd;
      bs.prep = call.ptr<PreintPrepared>(o_pp);
      VILO_HIP(hipMemsetAsync(bs.prep, 0, sizeof(PreintPrepared) * NF, ctx->stream));
      if (vilo_launch_prepare_preint_imu(ctx, (int)NF, (const vilo_preint_imu *)R.d_pre, bs.prep, bd.prep_bad, a.prep_skip, 1) != VILO_OK) return VILO_ERR_HIP;
      if (vilo_launch_embed_sqrt15(ctx, bs) != VILO_OK) return VILO_ERR_HIP;
      hipLaunchKernelGGL(k_reprop_commit, dim3((unsigned)NF), dim3(RP_THREADS), 0, ctx->stream, (int)NF, (int)(sizeof(PreintPrepared) / sizeof(double)), (const double *)bs.prep,
                         (double *)bd.prep, (const int *)a.go, (int *)nullptr);
    }
    if (R.replaced(ctx, bd) != VILO_OK) return VILO_ERR_HIP;
  }
  VILO_HIP(call.finish());
  std::vector<vilo_interval_reprop_record> host(NF);
  VILO_HIP(call.down(host.data(), a.out, sizeof(vilo_interval_reprop_record) * NF));
  if (records) memcpy(records, host.data(), sizeof(vilo_interval_reprop_record) * NF);
  if (wr) {
    bool all_live = true;
    for (const vilo_interval_reprop_record &r : host) all_live = all_live && (r.status == VILO_REPROP_OK || r.status == VILO_REPROP_NO_INTERVAL);
    R.full(all_live);
  }
  return VILO_OK;
}

extern "C" int vilo_window_repropagate(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_sample *samples,
                                       const int32_t *offsets, const vilo_reprop_opts *opts, const double *lin, const uint8_t *mask,
                                       vilo_interval_reprop_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_reprop_opts o;
  const int rc0 = reprop_check_opts(ctx, opts, samples, offsets, lin, mask, &o);
  if (rc0 != VILO_OK) return rc0;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) -> int {
    const size_t NF = (size_t)n_windows * 10;
    std::vector<vilo_interval_reprop_record> rec(NF);
    int rc = vilo_batch_repropagate(ctx, bt, samples, offsets, &o, lin, mask, rec.data());
    if (rc != VILO_OK) return rc;
    if (records) memcpy(records, rec.data(), sizeof(vilo_interval_reprop_record) * NF);
    if (!o.write) return rc;
    // the records this call wrote, and only those (the others are on the device in the form they went up in), into the caller's arrays
    const BatchRecords &R = bt->rec;
    const size_t rec_bytes = R.leg ? sizeof(vilo_preint) : sizeof(vilo_preint_imu);
    for (size_t f = 0; f < NF; ++f) {
      if (rec[f].status != VILO_REPROP_OK || !rec[f].selected) continue;
      const vilo_window_desc &d = in[f / 10];
      void *dst = R.leg ? (void *)(d.preint + f % 10) : (void *)(d.preint_imu + f % 10);
      VILO_HIP(hipMemcpy(dst, (const char *)R.d_pre + rec_bytes * f, rec_bytes, hipMemcpyDeviceToHost));
    }
    return rc;
  });
}

extern "C" double vilo_last_repropagate_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_reprop_ms : -1.0; }
