// Covariance of a frame's state carried through IMU samples (vilo_batch_dead_reckon_covariance, include/vilo_gpu.h): the error-state
// recurrence of IntegrationBase::midPointIntegration (integration_base.h:103-137), Sigma <- F Sigma F^T + V Q V^T, in the world frame,
// beside the nominal state of vilo_batch_dead_reckon (kernels_deadreckon.hip), whose arithmetic the nominal chain here repeats to the bit.
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_dr_covariance  16 lanes = one window, four windows per wave, one wave per workgroup. Lane j of a window holds column j of Sigma
//                    (15 doubles; lane 15 is the padding column and stays zero), and every lane runs the window's nominal chain itself
//                    (the same values in all sixteen: nothing of it crosses lanes). F is block-sparse: with AB = R0 [a0]x + R1 [a1]x K,
//                    S = R0 + R1, C = R1 [a1]x and K = I - [w]x dt (five 3 x 3 matrices, formed once per step) F c is four 3 x 3
//                    matrix-vector products and a few scaled sums (f_times), not a 15 x 15 product. A step is
//                      M = F Sigma          column by column: lane-local
//                      M^T                  through LDS: lane j writes its column, reads row j (a 16 x 17 tile per window: column
//                                           stride 17 doubles, so the 8-byte reads of a half-wave fall on 32 distinct bank pairs)
//                      Sigma' = F M^T       lane-local again (Sigma is symmetric to rounding, so M^T = Sigma F^T)
//                      + V Q V^T e_j        lane-local: the lane selects row j of V (R0, R1, C rows scaled) and applies V to Q times it
//                    The only exchange is inside the window's 16 lanes of one wave (no __syncthreads, no atomics), so windows of
//                    different range lengths that share a wave do not meet: their loops diverge and each touches its own LDS tile.
//                    Whether a window is finite is agreed over its 16 lanes by one ballot after the loop (sigma_column.hpp).
// The alternative, a wave per window with the padded 16 x 16 products on the matrix cores (four v_mfma_f64_16x16x4 per factor), spends
// 2 x 4096 multiply-adds per step on products of which F's sparsity leaves about 1300 (16 lanes x (2 x 36 + 9)), moves both operands
// through LDS or lane permutes every step, and gives a wave's 64 nominal chains to one window; DESIGN §4.29 has the figures.
//
// Floating-point contraction is off for the whole file, the inlined helpers of vilo_math.hpp included: state_out must be bit for bit
// k_dead_reckon's. The covariance arithmetic asks for its fused multiply-adds by name (fma()): the same in every lane and every batch.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "drcov_host.hpp"
#include "sigma_column.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_dr_cov_opts) == 8, "vilo_dr_cov_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_dead_reckon_record) == 8, "vilo_window_dead_reckon_record: 8 bytes (include/vilo_gpu.h)");

#define DRC_THREADS 64   // one wave
#define DRC_LANES 16     // lanes of a window
#define DRC_WPB (DRC_THREADS / DRC_LANES)
#define DRC_LD 17        // doubles between two rows of a window's LDS tile

struct DrCovArgs {
  int from_frame, pad;
  double g_norm;
  double q[DRC_NOISE];          // variances of the noise blocks (dr_cov_noise)
  const double *rows;           // [n_samples][DR_ROW] packed samples
  const int *offsets;           // [W + 1]
  const int *step_offsets;      // [W + 1]
  const double *cov_in;         // [W][15][15], or null
  double *state;                // [W][DR_STATE]
  double *cov;                  // [W][15][15]
  double *traj;                 // [sum n_steps][6][6], or null
  vilo_window_dead_reckon_record *rec;   // [W]
};

namespace {

using vilo::m3;
using vilo::v3;

__device__ __forceinline__ bool drc_finite3(const v3 &v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }
// M v with fused multiply-adds
__device__ __forceinline__ v3 drc_mv(const m3 &M, const v3 &v) {
  return vilo::mk3(fma(M.a[2], v.z, fma(M.a[1], v.y, M.a[0] * v.x)), fma(M.a[5], v.z, fma(M.a[4], v.y, M.a[3] * v.x)),
                   fma(M.a[8], v.z, fma(M.a[7], v.y, M.a[6] * v.x)));
}
__device__ __forceinline__ m3 drc_mm(const m3 &A, const m3 &B) {
  m3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) o.a[3 * r + c] = fma(A.a[3 * r + 2], B.a[6 + c], fma(A.a[3 * r + 1], B.a[3 + c], A.a[3 * r] * B.a[c]));
  return o;
}
// R [v]x: row r is (row r of R) x v
__device__ __forceinline__ m3 drc_mul_skew(const m3 &R, const v3 &v) {
  m3 o;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double r0 = R.a[3 * r], r1 = R.a[3 * r + 1], r2 = R.a[3 * r + 2];
    o.a[3 * r] = fma(r1, v.z, -(r2 * v.y));
    o.a[3 * r + 1] = fma(r2, v.x, -(r0 * v.z));
    o.a[3 * r + 2] = fma(r0, v.y, -(r1 * v.x));
  }
  return o;
}
// row jj of M (jj differs between lanes: selects, not an indexed register array)
__device__ __forceinline__ v3 drc_row(const m3 &M, int jj) {
  return vilo::mk3(sigcol_pick(jj, M.a[0], M.a[3], M.a[6]), sigcol_pick(jj, M.a[1], M.a[4], M.a[7]), sigcol_pick(jj, M.a[2], M.a[5], M.a[8]));
}

// The step's matrices: F and V are made of these and of dt (include/vilo_gpu.h writes the blocks out)
struct DrcStep {
  m3 AB, S, C, K, R0, R1;
  double dt, a, h;   // a = dt^2 / 4, h = dt / 2
};

// c <- F c
__device__ __forceinline__ void drc_f_times(const DrcStep &s, double *c) {
  const v3 p = vilo::ld3(c), th = vilo::ld3(c + 3), v = vilo::ld3(c + 6), ba = vilo::ld3(c + 9), bg = vilo::ld3(c + 12);
  const v3 t1 = drc_mv(s.AB, th), t2 = drc_mv(s.S, ba), t3 = drc_mv(s.C, bg), kt = drc_mv(s.K, th);
  // u = (A + C K) theta + (R0 + R1) ba - dt C bg: rows 0 and 6 of F are p + dt v - a u and v - h u
  const v3 u = vilo::mk3(fma(-s.dt, t3.x, t1.x + t2.x), fma(-s.dt, t3.y, t1.y + t2.y), fma(-s.dt, t3.z, t1.z + t2.z));
  c[0] = fma(-s.a, u.x, fma(s.dt, v.x, p.x)); c[1] = fma(-s.a, u.y, fma(s.dt, v.y, p.y)); c[2] = fma(-s.a, u.z, fma(s.dt, v.z, p.z));
  c[3] = fma(-s.dt, bg.x, kt.x); c[4] = fma(-s.dt, bg.y, kt.y); c[5] = fma(-s.dt, bg.z, kt.z);
  c[6] = fma(-s.h, u.x, v.x); c[7] = fma(-s.h, u.y, v.y); c[8] = fma(-s.h, u.z, v.z);
  // rows 9 .. 14: the biases' own
}

// c += V Q V^T e_j for the lane's column j = 3 blk + jj (blk 5: the padding column, nothing)
__device__ __forceinline__ void drc_add_noise(const DrcStep &s, const double *q, int blk, int jj, double *c) {
  // row j of V: [sc R0_jj | g | sc R1_jj | g | e_jj dt (blk 3) | e_jj dt (blk 4)], sc = a (dp rows), h (dv rows), 0; g = -sc h C_jj or (dtheta rows) h e_jj
  const double sc = blk == 0 ? s.a : (blk == 2 ? s.h : 0.0);
  const v3 e = vilo::mk3(jj == 0 ? 1.0 : 0.0, jj == 1 ? 1.0 : 0.0, jj == 2 ? 1.0 : 0.0);
  const v3 r0 = drc_row(s.R0, jj) * sc, r1 = drc_row(s.R1, jj) * sc;
  const v3 gc = drc_row(s.C, jj) * (-(sc * s.h)), ge = e * s.h;
  const v3 g = blk == 1 ? ge : gc;
  // Q times it; the two gyroscope blocks (columns 3 and 9 of V) are equal, so their contributions add up to twice one
  const v3 w0 = r0 * q[0], w2 = r1 * q[2], wg = g * q[1] + g * q[3];
  // V times that: rows dp = a t, dtheta = h wg, dv = h t with t = R0 w0 + R1 w2 - h C wg
  const v3 x0 = drc_mv(s.R0, w0), x2 = drc_mv(s.R1, w2), xg = drc_mv(s.C, wg);
  const v3 t = vilo::mk3(fma(-s.h, xg.x, x0.x + x2.x), fma(-s.h, xg.y, x0.y + x2.y), fma(-s.h, xg.z, x0.z + x2.z));
  const bool pv = blk <= 2;   // (the bias columns of V Q V^T have no entry in the dp, dtheta, dv rows)
  if (pv) {
    c[0] = fma(s.a, t.x, c[0]); c[1] = fma(s.a, t.y, c[1]); c[2] = fma(s.a, t.z, c[2]);
    c[3] = fma(s.h, wg.x, c[3]); c[4] = fma(s.h, wg.y, c[4]); c[5] = fma(s.h, wg.z, c[5]);
    c[6] = fma(s.h, t.x, c[6]); c[7] = fma(s.h, t.y, c[7]); c[8] = fma(s.h, t.z, c[8]);
  }
  const double na = s.dt * (q[4] * s.dt), ng = s.dt * (q[5] * s.dt);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    if (blk == 3 && jj == i) c[9 + i] += na;
    if (blk == 4 && jj == i) c[12 + i] += ng;
  }
}

}  // namespace

__global__ void __launch_bounds__(DRC_THREADS) k_dr_covariance(BatchDev b, DrCovArgs a) {
  using namespace vilo;
  __shared__ double tile[DRC_WPB * DRC_LANES * DRC_LD];
  const int j = threadIdx.x & (DRC_LANES - 1), grp = threadIdx.x / DRC_LANES;
  const int win = blockIdx.x * DRC_WPB + grp;
  if (win >= b.W) return;   // (whole windows: the wave's other windows go on; nothing below waits for a workgroup)
  double *T = tile + grp * DRC_LANES * DRC_LD;
  const int blk = j / 3, jj = j - 3 * blk;
  const SampleRange rg(b, win, a.from_frame, a.offsets);
  double *traj = rg.trajectory(a.traj, DRC_POSE * DRC_POSE, a.step_offsets, win);
  const double *x = b.x + (size_t)win * XSTRIDE;

  // row j of the tile: what lane 15 reads back every step is these zeros (row 15 is never written)
#pragma unroll
  for (int k = 0; k < DRC_LD; ++k) T[DRC_LD * j + k] = 0.0;

  bool finite = true;
  double c[DRC_N];   // column j of Sigma
#pragma unroll
  for (int i = 0; i < DRC_N; ++i) c[i] = 0.0;
  double so[DR_STATE];
#pragma unroll
  for (int i = 0; i < DR_STATE; ++i) so[i] = 0.0;
  if (!rg.no_frame) {
    if (a.cov_in && j < DRC_N) {
      // the upper triangle alone: entry (i, j) for i <= j, (j, i) for the mirrored rest
      const double *ci = a.cov_in + (size_t)(DRC_N * DRC_N) * win;
#pragma unroll
      for (int i = 0; i < DRC_N; ++i) {
        c[i] = i <= j ? ci[DRC_N * i + j] : ci[DRC_N * j + i];
        finite = finite && isfinite(c[i]);
      }
    }
    // the nominal chain: k_dead_reckon's, operation by operation (kernels_deadreckon.hip); why the two are not one function: DESIGN 4.36
    const double *pose = x + XO_POSE + 7 * rg.f, *sb = x + XO_SB + 9 * rg.f;
    v3 P = ld3(pose), V = ld3(sb);
    const v3 ba = ld3(sb + 3), bg = ld3(sb + 6);
    const quat q0 = ldq_pose(pose);
    finite = finite && drc_finite3(P) && drc_finite3(V) && drc_finite3(ba) && drc_finite3(bg) && isfinite(q0.w) && isfinite(q0.x) && isfinite(q0.y) && isfinite(q0.z);
    m3 R = qR(qnormalized(q0));
    const v3 g = mk3(0.0, 0.0, a.g_norm);
    if (rg.n_steps > 0) {
      const double *row = a.rows + (size_t)DR_ROW * rg.s_begin;
      v3 acc_0 = ld3(row + 1), gyr_0 = ld3(row + 4);
      finite = finite && drc_finite3(acc_0) && drc_finite3(gyr_0);
      double nxt[DR_ROW];
#pragma unroll
      for (int k = 0; k < DR_ROW; ++k) nxt[k] = row[DR_ROW + k];
      for (int i = 1; i < rg.n; ++i) {
        double cur[DR_ROW];
#pragma unroll
        for (int k = 0; k < DR_ROW; ++k) cur[k] = nxt[k];
        if (i + 1 < rg.n) {
          const double *nr = row + (size_t)DR_ROW * (i + 1);
#pragma unroll
          for (int k = 0; k < DR_ROW; ++k) nxt[k] = nr[k];
        }
        const double dt = cur[0];
        const v3 acc_1 = ld3(cur + 1), gyr_1 = ld3(cur + 4);
        finite = finite && isfinite(dt) && drc_finite3(acc_1) && drc_finite3(gyr_1);
        DrcStep s;
        s.R0 = R;
        // estimator.cpp:640-646
        const v3 un_acc_0 = R * (acc_0 - ba) - g;
        const v3 un_gyr = (gyr_0 + gyr_1) * 0.5 - bg;
        R = R * qR(deltaQ(un_gyr * dt));
        const v3 un_acc_1 = R * (acc_1 - ba) - g;
        const v3 un_acc = (un_acc_0 + un_acc_1) * 0.5;
        P = P + (V * dt + un_acc * (0.5 * dt * dt));
        V = V + un_acc * dt;
        // integration_base.h:87-132 at R0 = the R before the update, R1 = the R after it
        s.R1 = R;
        s.dt = dt; s.a = 0.25 * dt * dt; s.h = 0.5 * dt;
        s.S = s.R0 + s.R1;
        s.C = drc_mul_skew(s.R1, acc_1 - ba);
        s.K.a[0] = 1.0; s.K.a[1] = un_gyr.z * dt; s.K.a[2] = -(un_gyr.y * dt);
        s.K.a[3] = -(un_gyr.z * dt); s.K.a[4] = 1.0; s.K.a[5] = un_gyr.x * dt;
        s.K.a[6] = un_gyr.y * dt; s.K.a[7] = -(un_gyr.x * dt); s.K.a[8] = 1.0;
        s.AB = drc_mul_skew(s.R0, acc_0 - ba) + drc_mm(s.C, s.K);
        acc_0 = acc_1; gyr_0 = gyr_1;

        drc_f_times(s, c);                       // column j of M = F Sigma
#pragma unroll
        for (int r = 0; r < DRC_N; ++r) T[DRC_LD * r + j] = c[r];
        sigcol_fence();
#pragma unroll
        for (int k = 0; k < DRC_N; ++k) c[k] = T[DRC_LD * j + k];   // row j of M: column j of Sigma F^T
        sigcol_fence();
        drc_f_times(s, c);                       // column j of F Sigma F^T
        drc_add_noise(s, a.q, blk, jj, c);
        if (traj) sigcol_store_sym<DRC_POSE>(traj + (size_t)(DRC_POSE * DRC_POSE) * (i - 1), c, j);
      }
    }
    const quat qo = quat_from_R_dev(R);
    so[0] = P.x; so[1] = P.y; so[2] = P.z; so[3] = qo.x; so[4] = qo.y; so[5] = qo.z; so[6] = qo.w; so[7] = V.x; so[8] = V.y; so[9] = V.z;
#pragma unroll
    for (int i = 0; i < DR_STATE; ++i) finite = finite && isfinite(so[i]);
#pragma unroll
    for (int i = 0; i < DRC_N; ++i) finite = finite && isfinite(c[i]);
  }
  // one verdict per window: its sixteen lanes'
  const int status = rg.status(sigcol_all_finite<DRC_LANES>(finite, grp));
  if (status != VILO_DR_OK) {
#pragma unroll
    for (int i = 0; i < DRC_N; ++i) c[i] = 0.0;
#pragma unroll
    for (int i = 0; i < DR_STATE; ++i) so[i] = 0.0;
    if (traj)
      for (int i = 0; i < rg.n_steps; ++i) sigcol_store_sym<DRC_POSE>(traj + (size_t)(DRC_POSE * DRC_POSE) * i, c, j);
  }
  sigcol_store_sym<DRC_N>(a.cov + (size_t)(DRC_N * DRC_N) * win, c, j);
  if (j == 0) {
    double2 *sp = (double2 *)(a.state + (size_t)DR_STATE * win);   // (80-byte rows of a 256-byte aligned block: 16-byte aligned)
#pragma unroll
    for (int i = 0; i < DR_STATE / 2; ++i) sp[i] = make_double2(so[2 * i], so[2 * i + 1]);
    rg.record(a.rec, win, status);
  }
}

extern "C" void vilo_default_dr_cov_opts(vilo_dr_cov_opts *o) {
  if (!o) return;
  o->from_frame = -1;
  o->reserved = 0;
}

static const char DR_COV_CALL[] = "vilo_batch_dead_reckon_covariance";

extern "C" int vilo_batch_dead_reckon_covariance(vilo_ctx *ctx, vilo_batch *bt, const vilo_dr_cov_opts *opts, const vilo_sample *samples,
                                                 const int32_t *offsets, const double *cov_in, double *state_out, double *cov_out,
                                                 double *pose_cov_trajectory, vilo_window_dead_reckon_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  const vilo_dr_cov_opts o = sample_call_opts(opts, vilo_default_dr_cov_opts);
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (const char *what = vilo::dr_cov_check(o, W, samples, offsets, state_out, cov_out)) return sample_call_fail(ctx, DR_COV_CALL, what, VILO_ERR_BAD_ARG);
  BatchCall call(ctx, bt, &vilo_ctx::last_dr_cov_ms);
  if (W == 0) return VILO_OK;
  SampleUpload up(ctx, call, DR_COV_CALL, W, samples, offsets, DR_ROW, vilo::dead_reckon_pack);
  if (!up.staged()) return VILO_ERR_HIP;
  const int32_t n_rows = up.n_rows;
  const vilo::DrCovCounts cnt = vilo::dr_cov_counts(W, n_rows);
  const bool want_traj = pose_cov_trajectory != nullptr;
  // the call's device memory after the samples': cov_in | states | covariances | trajectory | records
  const size_t o_i = call.lay.take<double>(cnt.cov, cov_in != nullptr), o_x = call.lay.take<double>(cnt.state), o_c = call.lay.take<double>(cnt.cov);
  const size_t o_j = call.lay.take<double>(cnt.traj, want_traj), o_r = call.lay.take<vilo_window_dead_reckon_record>(cnt.rec);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(up.send(call));
  DrCovArgs a;
  a.from_frame = o.from_frame; a.pad = 0;
  a.g_norm = ctx->cfg.g_norm;
  vilo::dr_cov_noise(ctx->cfg, a.q);
  a.rows = up.rows;
  a.offsets = up.offsets;
  a.step_offsets = up.step_offsets;
  a.cov_in = cov_in ? call.ptr<double>(o_i) : nullptr;
  a.state = call.ptr<double>(o_x);
  a.cov = call.ptr<double>(o_c);
  a.traj = want_traj && n_rows > 0 ? call.ptr<double>(o_j) : nullptr;
  a.rec = call.ptr<vilo_window_dead_reckon_record>(o_r);
  if (cov_in) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_i), cov_in, sizeof(double) * cnt.cov, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_dr_covariance, dim3((W + DRC_WPB - 1) / DRC_WPB), dim3(DRC_THREADS), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(state_out, a.state, sizeof(double) * cnt.state));
  VILO_HIP(call.down(cov_out, a.cov, sizeof(double) * cnt.cov));
  if (want_traj) VILO_HIP(call.down(pose_cov_trajectory, a.traj, sizeof(double) * cnt.traj));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_dead_reckon_record) * cnt.rec));
  return VILO_OK;
}

extern "C" int vilo_window_dead_reckon_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                                  const vilo_dr_cov_opts *opts, const vilo_sample *samples, const int32_t *offsets,
                                                  const double *cov_in, double *state_out, double *cov_out, double *pose_cov_trajectory,
                                                  vilo_window_dead_reckon_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  const vilo_dr_cov_opts o = sample_call_opts(opts, vilo_default_dr_cov_opts);
  if (const char *what = vilo::dr_cov_check(o, n_windows, samples, offsets, state_out, cov_out)) return sample_call_fail(ctx, DR_COV_CALL, what, VILO_ERR_BAD_ARG);
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_dead_reckon_covariance(ctx, bt, &o, samples, offsets, cov_in, state_out, cov_out, pose_cov_trajectory, records);
  });
}

extern "C" double vilo_last_dr_cov_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_dr_cov_ms : -1.0; }
