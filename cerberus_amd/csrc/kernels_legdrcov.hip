// Covariance of a frame's leg-odometry state carried through samples (vilo_batch_leg_dead_reckon_covariance, include/vilo_gpu.h): the
// error-state recurrence of IMULegIntegrationBase::midPointIntegration (imu_leg_integration_base.cpp:288-468), Sigma <- F Sigma F^T +
// V Q V^T over 31 coordinates, in the world frame, beside the nominal state of vilo_batch_leg_dead_reckon (kernels_legdr.hip), which is
// legdr_host.hpp's legdr_step, called here as there. The blocks of F and V and the two products are legdrcov_host.hpp's, the functions the
// CPU path calls too.
//
// One launch, one code path for every batch size (no launch plan, no switch; no output depends on the batch a window shares, nor on its
// position):
//   k_leg_dr_covariance  32 lanes = one window, two windows per wave, one wave per workgroup. Lane j of a window holds column j of Sigma
//                        (31 doubles; lane 31 is the padding column and stays zero). Between steps the column rests in the window's
//                        tile in LDS: held in registers across the nominal step it would cost the lane a spill to scratch. A step:
//                          nominal   every quad of the window runs legdr_step<LegDrQuadLane> for leg (lane & 3): the same values in the
//                                    same order in all eight quads, so delta_q, result_delta_q, delta_v and the flags are in every
//                                    lane's registers and nothing of them crosses lanes but the quad's own DPP reads
//                          blocks    a lane cannot hold the operands of four legs x two endpoints: lanes 0 .. 3 (one leg each) store
//                                    their leg's sample terms (v, p, h, R_br J, g: 27 doubles; a sample is the second endpoint of one
//                                    step and the first of the next, so two slots alternate), its rows of F - I and V and its noise
//                                    into the window's step block in LDS; lane 0 stores the dp, dtheta, dv rows as well
//                          M = F Sigma       column by column, lane-local: 165 fused multiply-adds on the 21 x 16 block that F - I is
//                                            (its entries are broadcast reads of LDS: every lane reads the same address)
//                          M^T               through LDS: lane j writes its column, reads row j (a 32 x 33 tile per window: row stride
//                                            33 doubles, so the 32 lanes' reads fall on distinct bank pairs)
//                          Sigma' = F M^T    lane-local again
//                          + V Q V^T e_j     lane-local: row j of V's dense part (21 x 24) times Q, then V times that; the -dt I blocks
//                                            of V add to the diagonal entry alone
//                        The only exchange is inside the window's 32 lanes of one wave (no __syncthreads, no atomics), so the two
//                        windows of a wave, whose ranges may differ in length, do not meet: their loops diverge and each touches its
//                        own LDS. Whether a window is finite is agreed over its 32 lanes by one ballot after the loop (sigma_column.hpp).
// The padded 32 x 32 x 32 products on the FP64 matrix cores were not built: F - I has 165 entries of 961 that are ever non-zero.
//
// Floating-point contraction is off for the whole file, the inlined helpers of vilo_math.hpp, legdr_host.hpp and legdrcov_host.hpp
// included: state_out and legs_out must be bit for bit k_leg_dead_reckon's. The covariance products ask for their fused multiply-adds by
// name (fma()): the same in every lane, in every batch and in the CPU path.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "legdr_quad.hpp"
#include "legdrcov_host.hpp"
#include "sigma_column.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_leg_dr_cov_opts) == 8, "vilo_leg_dr_cov_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_leg_dead_reckon_record) == 8, "vilo_window_leg_dead_reckon_record: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_sample) == 8 * LEGDR_ROW, "a packed row is a vilo_sample in another order");

#define LDCK_THREADS 64   // one wave
#define LDCK_LANES 32     // lanes of a window
#define LDCK_WPB (LDCK_THREADS / LDCK_LANES)
#define LDCK_LD 33        // doubles between two rows of a window's transposition tile
#define LDCK_TILE (LDCK_LANES * LDCK_LD)

struct LegDrCovArgs {
  int from_frame, pad;
  const double *rows;           // [n_samples][LEGDR_ROW] packed samples
  const int *offsets;           // [W + 1]
  const int *step_offsets;      // [W + 1]
  const double *cov_in;         // [W][19][19], or null
  double *state;                // [W][LEGDR_STATE]
  double *legs;                 // [W][LEGDR_LEGS]
  double *cov;                  // [W][31][31]
  double *pose_traj;            // [sum n_steps][6][6], or null
  double *leg_traj;             // [sum n_steps][4][3][3], or null
  vilo_window_leg_dead_reckon_record *rec;   // [W]
};

namespace {

using vilo::LDC_O_BA;
using vilo::LDC_O_EPS;

// The 3 x 3 diagonal block of deps_l from the lanes 9 .. 20 (column 9 + 3 l + jj): values selected, not addresses (c is in registers)
__device__ __forceinline__ void ldck_store_legs(double *dst /* [4][3][3] */, const double *c, int j) {
  if (j < LDC_O_EPS || j >= LDC_O_BA) return;
  const int l = (j - LDC_O_EPS) / 3, jj = (j - LDC_O_EPS) - 3 * l;
#pragma unroll
  for (int ii = 0; ii < 3; ++ii) {
    const double v = sigcol_pick(l, c[LDC_O_EPS + ii], c[LDC_O_EPS + 3 + ii], c[LDC_O_EPS + 6 + ii], c[LDC_O_EPS + 9 + ii]);
    if (ii <= jj) {
      dst[9 * l + 3 * ii + jj] = v;
      dst[9 * l + 3 * jj + ii] = v;
    }
  }
}

}  // namespace

__global__ void __launch_bounds__(LDCK_THREADS) k_leg_dr_covariance(BatchDev b, const vilo_config *cfgp, LegDrCovArgs a) {
  using namespace vilo;
  __shared__ double lds[LDCK_WPB * (LDCK_TILE + LDC_SB_TOTAL)];
  const int j = threadIdx.x & (LDCK_LANES - 1), grp = threadIdx.x / LDCK_LANES;
  const int win = blockIdx.x * LDCK_WPB + grp;
  if (win >= b.W) return;   // (whole windows: the wave's other window goes on; nothing below waits for a workgroup)
  double *T = lds + grp * (LDCK_TILE + LDC_SB_TOTAL), *sb = T + LDCK_TILE;
  LegDrQuadLane x;
  x.j = j & 3;
  const bool owner = j < 4;   // the lane that stores leg j's blocks; lane 0 the shared ones
  const vilo_config &cfg = *cfgp;
  const int n_frames = b.win[win].n_frames;
  const int f = a.from_frame < 0 ? n_frames - 1 : a.from_frame;
  const int s_begin = a.offsets[win], n = a.offsets[win + 1] - s_begin;
  const int n_steps = n > 1 ? n - 1 : 0;
  double *state = a.state + (size_t)LEGDR_STATE * win, *legs = a.legs + (size_t)LEGDR_LEGS * win;
  double *pose_traj = a.pose_traj ? a.pose_traj + (size_t)(LDC_POSE * LDC_POSE) * a.step_offsets[win] : nullptr;
  double *leg_traj = a.leg_traj ? a.leg_traj + (size_t)LDC_LEGCOV * a.step_offsets[win] : nullptr;
  const double *xs = b.x + (size_t)win * XSTRIDE;

  // the window's LDS: zeros (row 31 of the tile, which lane 31 reads back every step, is never written again; the entries of the step
  // block that are zero in every step neither), then the constant variances
  LdcNoise q;
  ldc_noise_const(cfg, q);
  for (int k = j; k < LDCK_TILE + LDC_SB_TOTAL; k += LDCK_LANES) T[k] = 0.0;
  sigcol_fence();
  if (j == 0) ldc_dense_noise(q, sb + LDC_SB_QD);
  sigcol_fence();

  const bool no_frame = f < 0 || f >= n_frames;   // (f <= VILO_MAX_FRAMES - 1 by the argument check)
  bool finite = true;
  double c[LDC_N];   // column j of Sigma
#pragma unroll
  for (int i = 0; i < LDC_N; ++i) c[i] = 0.0;
  if (!no_frame) {
    if (a.cov_in && j < LDC_N) {
      const double *ci = a.cov_in + (size_t)(LDC_IN * LDC_IN) * win;
#pragma unroll
      for (int i = 0; i < LDC_N; ++i) {
        c[i] = ldc_sigma0(ci, i, j);
        finite = finite && legdr_finite(c[i]);
      }
    }
    // Sigma rests in the tile (column j down the lane's tile column) while the nominal step and the blocks are at work: the registers of
    // a lane do not hold both
#pragma unroll
    for (int r = 0; r < LDC_N; ++r) T[LDCK_LD * r + j] = c[r];
    // the nominal chain: k_leg_dead_reckon's, call by call (kernels_legdr.hip), and the window's range, written out here: through
    // legdr_window_start / legdr_next_row and SampleRange this kernel, at 256 VGPRs, ran 3 % slower
    const double *pose = xs + XO_POSE + 7 * f, *sbs = xs + XO_SB + 9 * f, *lb = xs + XO_LB + 4 * f;
    finite = finite && legdr_finite(lb[x.j]);
#pragma unroll
    for (int k = 0; k < 7; ++k) finite = finite && legdr_finite(pose[k]);
#pragma unroll
    for (int k = 3; k < 9; ++k) finite = finite && legdr_finite(sbs[k]);
    LegDrConst lc;
    legdr_const(cfg, sbs + 3, sbs + 6, lc);
    LegDrWorld wf;
    wf.R0 = qR(qnormalized(ldq_pose(pose)));
    wf.P0 = ld3(pose);
    LegDrState<1> s;
    LegDrStep<1> o;
    o.flag[0] = 0.0;
    if (n_steps > 0) {
      const double *row = a.rows + (size_t)LEGDR_ROW * s_begin;
      const double *mine = row + LEGDR_ROW_SHARED + LEGDR_ROW_LEG * x.j;
      double sh[LEGDR_ROW_SHARED], lg[1][LEGDR_ROW_LEG];
      sh[0] = 0.0;
#pragma unroll
      for (int k = 1; k < LEGDR_ROW_SHARED; ++k) sh[k] = row[k];
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_LEG; ++k) lg[0][k] = mine[k];
#pragma unroll
      for (int k = 1; k < LEGDR_ROW_SHARED; ++k) finite = finite && legdr_finite(sh[k]);
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_LEG; ++k) finite = finite && legdr_finite(lg[0][k]);
      legdr_start(lc, cfg, lb, sh, lg, x, s);
      if (owner) ldc_sample_terms(lc, s.gyr0, lg[0], s.rho[0], s.rf[0], s.v0[0], sb + ldc_terms_at(0, x.j));
      for (int i = 1; i < n; ++i) {
        const size_t at = (size_t)LEGDR_ROW * i;
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_SHARED; ++k) sh[k] = row[at + k];
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_LEG; ++k) lg[0][k] = mine[at + k];
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_SHARED; ++k) finite = finite && legdr_finite(sh[k]);
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_LEG; ++k) finite = finite && legdr_finite(lg[0][k]);
        const quat dq0 = s.dq;
        const v3 dv0 = s.dv, acc0 = s.acc0, gyr0 = s.gyr0;
        legdr_step(lc, s, sh, lg, x, o);
        // the step's blocks, from the nominal step's own values
        const double dt = sh[0];
        double f4[4];
        x.gather(o.flag, f4);
        const bool all_air = f4[0] + f4[1] + f4[2] + f4[3] < 1e-6;
        if (owner) {
          const m3 R0 = wf.R0 * qR(dq0), R1 = wf.R0 * qR(o.rq);
          const m3 K = ldc_kappa7(0.5 * (gyr0 + s.gyr0) - lc.bg, dt);
          const double *t0 = sb + ldc_terms_at((i - 1) & 1, x.j);
          double *t1 = sb + ldc_terms_at(i & 1, x.j);
          ldc_sample_terms(lc, s.gyr0, lg[0], s.rho[0], s.rf[0], s.v0[0], t1);
          double unc[3], rho_unc;
          ldc_leg_uncertainty(lc, q, o.flag[0], s.ff_var[0], o.lo_v[0], dv0, all_air, unc, rho_unc);
          ldc_leg_noise(wf.R0, dt, unc, rho_unc, x.j, sb);
          ldc_leg_rows(R0, R1, K, dt, t0, t1, x.j, sb);
          if (j == 0) ldc_imu_rows(R0, R1, K, acc0 - lc.ba, s.acc0 - lc.ba, dt, q, sb);
        }
        sigcol_fence();
#pragma unroll
        for (int r = 0; r < LDC_N; ++r) c[r] = T[LDCK_LD * r + j];
        ldc_f_times(sb, c);                      // column j of M = F Sigma
#pragma unroll
        for (int r = 0; r < LDC_N; ++r) T[LDCK_LD * r + j] = c[r];
        sigcol_fence();
#pragma unroll
        for (int k = 0; k < LDC_N; ++k) c[k] = T[LDCK_LD * j + k];   // row j of M: column j of Sigma F^T
        sigcol_fence();
        ldc_f_times(sb, c);                      // column j of F Sigma F^T
        ldc_add_noise(sb, j, c);
#pragma unroll
        for (int r = 0; r < LDC_N; ++r) T[LDCK_LD * r + j] = c[r];
        sigcol_fence();                            // (the next step's blocks are stored after this step's were read)
        if (pose_traj) sigcol_store_sym<LDC_POSE>(pose_traj + (size_t)(LDC_POSE * LDC_POSE) * (i - 1), c, j);
        if (leg_traj) ldck_store_legs(leg_traj + (size_t)LDC_LEGCOV * (i - 1), c, j);
      }
    } else {
      legdr_start(lc, cfg, lb, (const double *)nullptr, (const double (*)[LEGDR_ROW_LEG])nullptr, x, s);
    }
    if (owner) {
      legdr_state_row(wf, s, o.flag, x, state, legs);
      finite = finite && legdr_rows_finite(state, legs, x);
    }
#pragma unroll
    for (int r = 0; r < LDC_N; ++r) {
      c[r] = T[LDCK_LD * r + j];
      finite = finite && legdr_finite(c[r]);
    }
  }
  // one verdict per window: its 32 lanes'
  const bool window_finite = sigcol_all_finite<LDCK_LANES>(finite, grp);
  const int status = no_frame ? VILO_DR_NO_FRAME : (window_finite ? VILO_DR_OK : VILO_DR_NUMERIC);
  if (status != VILO_DR_OK) {
#pragma unroll
    for (int i = 0; i < LDC_N; ++i) c[i] = 0.0;
    if (owner) {   // (the lanes that wrote them)
      for (int i = x.j; i < LEGDR_STATE; i += 4) state[i] = 0.0;
      for (int i = x.j; i < LEGDR_LEGS; i += 4) legs[i] = 0.0;
    }
    if (pose_traj)
      for (size_t i = j; i < (size_t)(LDC_POSE * LDC_POSE) * n_steps; i += LDCK_LANES) pose_traj[i] = 0.0;
    if (leg_traj)
      for (size_t i = j; i < (size_t)LDC_LEGCOV * n_steps; i += LDCK_LANES) leg_traj[i] = 0.0;
  }
  sigcol_store_sym<LDC_N>(a.cov + (size_t)(LDC_N * LDC_N) * win, c, j);
  if (j == 0) {
    vilo_window_leg_dead_reckon_record r;
    r.n_steps = n_steps;
    r.status = status;
    a.rec[win] = r;
  }
}

extern "C" void vilo_default_leg_dr_cov_opts(vilo_leg_dr_cov_opts *o) {
  if (!o) return;
  o->from_frame = -1;
  o->reserved = 0;
}

static const char LEG_DR_COV_CALL[] = "vilo_batch_leg_dead_reckon_covariance";

extern "C" int vilo_batch_leg_dead_reckon_covariance(vilo_ctx *ctx, vilo_batch *bt, const vilo_leg_dr_cov_opts *opts, const vilo_sample *samples,
                                                     const int32_t *offsets, const double *cov_in, double *state_out, double *legs_out,
                                                     double *cov_out, double *pose_cov_trajectory, double *leg_cov_trajectory,
                                                     vilo_window_leg_dead_reckon_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  const vilo_leg_dr_cov_opts o = sample_call_opts(opts, vilo_default_leg_dr_cov_opts);
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (const char *what = vilo::leg_dr_cov_check(o, W, samples, offsets, state_out, legs_out, cov_out)) return sample_call_fail(ctx, LEG_DR_COV_CALL, what, VILO_ERR_BAD_ARG);
  BatchCall call(ctx, bt, &vilo_ctx::last_leg_dr_cov_ms);
  if (W == 0) return VILO_OK;
  if (!bt->rec.leg) return sample_call_fail(ctx, LEG_DR_COV_CALL, "the batch's windows have no leg factors (use_leg == 0)", VILO_ERR_UNSUPPORTED);
  SampleUpload up(ctx, call, LEG_DR_COV_CALL, W, samples, offsets, LEGDR_ROW, vilo::leg_dead_reckon_pack);
  if (!up.staged()) return VILO_ERR_HIP;
  const int32_t n_rows = up.n_rows;
  const vilo::LegDrCovCounts cnt = vilo::leg_dr_cov_counts(W, n_rows);
  const bool want_pose = pose_cov_trajectory != nullptr, want_leg = leg_cov_trajectory != nullptr;
  // the call's device memory after the samples': cov_in | states | legs | covariances | trajectories | records
  const size_t o_i = call.lay.take<double>(cnt.cov_in, cov_in != nullptr), o_x = call.lay.take<double>(cnt.state), o_l = call.lay.take<double>(cnt.legs);
  const size_t o_c = call.lay.take<double>(cnt.cov), o_p = call.lay.take<double>(cnt.pose_traj, want_pose), o_g = call.lay.take<double>(cnt.leg_traj, want_leg);
  const size_t o_r = call.lay.take<vilo_window_leg_dead_reckon_record>(cnt.rec);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(up.send(call));
  LegDrCovArgs a;
  a.from_frame = o.from_frame; a.pad = 0;
  a.rows = up.rows;
  a.offsets = up.offsets;
  a.step_offsets = up.step_offsets;
  a.cov_in = cov_in ? call.ptr<double>(o_i) : nullptr;
  a.state = call.ptr<double>(o_x);
  a.legs = call.ptr<double>(o_l);
  a.cov = call.ptr<double>(o_c);
  a.pose_traj = want_pose && n_rows > 0 ? call.ptr<double>(o_p) : nullptr;
  a.leg_traj = want_leg && n_rows > 0 ? call.ptr<double>(o_g) : nullptr;
  a.rec = call.ptr<vilo_window_leg_dead_reckon_record>(o_r);
  if (cov_in) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_i), cov_in, sizeof(double) * cnt.cov_in, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_leg_dr_covariance, dim3((W + LDCK_WPB - 1) / LDCK_WPB), dim3(LDCK_THREADS), 0, ctx->stream, bd,
                     (const vilo_config *)ctx->d_cfg, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(state_out, a.state, sizeof(double) * cnt.state));
  VILO_HIP(call.down(legs_out, a.legs, sizeof(double) * cnt.legs));
  VILO_HIP(call.down(cov_out, a.cov, sizeof(double) * cnt.cov));
  if (want_pose) VILO_HIP(call.down(pose_cov_trajectory, a.pose_traj, sizeof(double) * cnt.pose_traj));
  if (want_leg) VILO_HIP(call.down(leg_cov_trajectory, a.leg_traj, sizeof(double) * cnt.leg_traj));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_leg_dead_reckon_record) * cnt.rec));
  return VILO_OK;
}

extern "C" int vilo_window_leg_dead_reckon_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                                      const vilo_leg_dr_cov_opts *opts, const vilo_sample *samples, const int32_t *offsets,
                                                      const double *cov_in, double *state_out, double *legs_out, double *cov_out,
                                                      double *pose_cov_trajectory, double *leg_cov_trajectory,
                                                      vilo_window_leg_dead_reckon_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  const vilo_leg_dr_cov_opts o = sample_call_opts(opts, vilo_default_leg_dr_cov_opts);
  if (const char *what = vilo::leg_dr_cov_check(o, n_windows, samples, offsets, state_out, legs_out, cov_out)) return sample_call_fail(ctx, LEG_DR_COV_CALL, what, VILO_ERR_BAD_ARG);
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_leg_dead_reckon_covariance(ctx, bt, &o, samples, offsets, cov_in, state_out, legs_out, cov_out, pose_cov_trajectory,
                                                 leg_cov_trajectory, records);
  });
}

extern "C" double vilo_last_leg_dr_cov_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_leg_dr_cov_ms : -1.0; }
