// Residuals of every window of a batch at its current device state, and the reference's landmark outlier / failure test
// (vilo_batch_residuals, include/vilo_gpu.h; Estimator::outliersRejection, estimator.cpp:1741-1798; FeatureManager::setDepth /
// removeFailures, feature_manager.cpp:142-171).
//
// Three launches, one code path for every batch size (no output depends on the batch a window shares, nor on its position); the cost's
// arithmetic is cost_eval.hpp's pieces:
//   k_resid_landmarks  one wave per packed visual wave, lane = landmark, walking the wave's frames at x / lambda. Per block the whitened
//                      residual (stored in the caller's observation row), rho and |r|^2; per landmark the reference's reprojection sum
//                      in its own order of operations (no td, no velocities, no sqrt_info) and the flags. Per-landmark values go to
//                      the caller's landmark order (lm_off + lm_perm): no floating-point atomics.
//   k_resid_imu        lane = factor for the raw residual, then lane = row of sqrt_info: the whitened vector and 1/2 |u|^2 per
//                      interval, whatever the window's solver state.
//   k_resid_window     one workgroup per window: the prior's cost from its normal-equation form (prior_H / prior_b0 / prior_c0), then
//                      the landmark sums in caller order (a fixed per-thread stride and tree) and the window record.
// With vilo_batch_set_samples in force the records are first integrated again at x by the marginalisation's pass (k_repropagate mode 0 +
// the preparation), on copies: the call hands those kernels a BatchDev whose records, prepared records, flags and contact-force filters
// point into the call's own memory, so the batch's are never written.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "accept_body.hpp"
#include "batch_call.hpp"
#include "lin_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_window_residual) == 136, "vilo_window_residual: 136 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_residual_opts) == 8, "vilo_residual_opts: 8 bytes (include/vilo_gpu.h)");

// per-landmark values the window pass sums (caller order)
struct ResidLm {
  double *cost, *reproj, *plain;   // [n_lm] 1/2 sum rho, reprojection error in pixels, 1/2 sum |r|^2
  int *nb, *nh;                    // [n_lm] residual blocks, of which in Huber's linear region
  unsigned char *flags;            // [n_lm]
};

__global__ void __launch_bounds__(64) k_resid_landmarks(BatchDev b, double sq, double huber_a, double focal, double thr, const int *obs_row,
                                                        ResidLm out, double *obs_res) {
  using namespace vilo;
  const WaveMeta wv = b.wave[blockIdx.x];
  const WinMeta wm = b.win[wv.win];
  const int lane = threadIdx.x;
  int cs[4], cn[4], ckm[4], cgo[4];
  const LaneSeg ls = lane_segment(wv, b.chunk, lane, cs, cn, ckm, cgo);
  if (!ls.active) return;
  const int n = wv.n_lanes, s = ls.s, gi = ls.gi, o = wm.lm_off + b.lm_perm[gi];
  const double *x = b.x + (size_t)wv.win * XSTRIDE;
  const double *obs = b.obs + wv.obs_off;
  const unsigned char *flg = b.flags + wv.flag_off;
  double *orow = obs_res ? obs_res + 4 * (size_t)obs_row[gi] : nullptr;
  const double lam = b.lam[gi];
  // the factors' form (cost_eval.hpp): td-compensated start-frame point, its world point once per landmark
  auto row = [&](int t, int r) { return obs_at(obs, n, lane, t, r); };
  const double td = x[XO_TD];
  const double *ex0 = x + XO_EX, *ex1 = x + XO_EX + 7;
  const quat qic = ldq_pose(ex0), qic2 = ldq_pose(ex1);
  const v3 tic = ld3(ex0), tic2 = ld3(ex1);
  const v3 p_i = start_point(row(0, OBS_LX), row(0, OBS_LY), row(0, OBS_LZ), row(0, OBS_LVX), row(0, OBS_LVY), row(0, OBS_TD), td, 1.0 / lam, qic, tic);
  const double *pose_s = x + XO_POSE + 7 * s;
  const v3 p_w = world_point(pose_s, p_i);
  // Estimator::reprojectionError's form: rotation matrices of the normalised quaternions, depth = 1 / inv_depth, raw points
  const m3 Ri = qR(qnormalized(ldq_pose(pose_s))), ric0 = qR(qnormalized(qic)), ric1 = qR(qnormalized(qic2));
  const v3 Pi = ld3(pose_s);
  const double depth = 1.0 / lam;
  const v3 uvi = mk3(row(0, OBS_LX), row(0, OBS_LY), row(0, OBS_LZ));
  const v3 pts_w = Ri * (ric0 * (uvi * depth) + tic) + Pi;
  double cost = 0.0, plain = 0.0, err = 0.0;
  int nb = 0, nh = 0, cnt = 0;
  auto block = [&](const v3 &pcj, double px, double py, double *rout) {
    const CamBlock cb = camera_block(pcj, px, py, sq, huber_a);
    cost += cb.rho0;
    plain += cb.s2;
    ++nb;
    if (cb.s2 > huber_a * huber_a) ++nh;
    if (rout) { rout[0] = cb.r0; rout[1] = cb.r1; }
  };
  auto reproj = [&](const m3 &Rj, const v3 &Pj, const m3 &ricj, const v3 &ticj, double ux, double uy) {
    const v3 pts_cj = tr(ricj) * (tr(Rj) * (pts_w - Pj) - ticj);
    const double rx = pts_cj.x / pts_cj.z - ux, ry = pts_cj.y / pts_cj.z - uy;
    err += sqrt(rx * rx + ry * ry);
    ++cnt;
  };
  for (int t = 0; t < wv.kmax; ++t) {
    const unsigned char fl = flg[(size_t)t * n + lane];
    if (!(fl & 1)) continue;
    double *rr = orow ? orow + 4 * (size_t)t : nullptr;
    const double dtj = td - row(t, OBS_TD);
    const double *pose_j = x + XO_POSE + 7 * min(s + t, VILO_MAX_FRAMES - 1);
    const m3 Rj = qR(qnormalized(ldq_pose(pose_j)));
    const v3 Pj = ld3(pose_j);
    v3 p_j = p_i;
    if (t > 0) {
      p_j = frame_point(pose_j, p_w);
      block(camera_point(qic, tic, p_j), row(t, OBS_LX) - row(t, OBS_LVX) * dtj, row(t, OBS_LY) - row(t, OBS_LVY) * dtj, rr);
      reproj(Rj, Pj, ric0, tic, row(t, OBS_LX), row(t, OBS_LY));
    } else if (rr) {
      rr[0] = NAN; rr[1] = NAN;
    }
    if (fl & 2) {
      block(camera_point(qic2, tic2, p_j), row(t, OBS_RX) - row(t, OBS_RVX) * dtj, row(t, OBS_RY) - row(t, OBS_RVY) * dtj, rr ? rr + 2 : nullptr);
      reproj(Rj, Pj, ric1, tic2, row(t, OBS_RX), row(t, OBS_RY));
    } else if (rr) {
      rr[2] = NAN; rr[3] = NAN;
    }
  }
  const double px = (err / cnt) * focal;
  out.cost[o] = 0.5 * cost;
  out.reproj[o] = px;
  out.plain[o] = 0.5 * plain;
  out.nb[o] = nb;
  out.nh[o] = nh;
  out.flags[o] = (unsigned char)((px > thr ? 1 : 0) | (depth < 0.0 ? 2 : 0) | (nh > 0 ? 4 : 0));
}

// one wave per 64 factors (imu_stage's tile); cost_out [W * 10], res_out [W * 10][31] or null
__global__ void __launch_bounds__(64) k_resid_imu(BatchDev b, double g_norm, double *cost_out, double *res_out) {
  using namespace vilo;
  __shared__ double rs[32 * 64];   // [entry][factor of the wave]; row 31: 1/2 |u|^2 per factor
  const int lane = threadIdx.x, f0 = blockIdx.x * 64, f = f0 + lane;
  const int NF = b.W * 10;
  bool live = false, bad = false;
  {
    ImuResid r = {};
    if (f < NF) {
      const int win = f / 10;
      live = !b.imu_skip[f];
      bad = live && b.prep_bad && b.prep_bad[f];
      if (live) r = imu_factor_raw(b, f, b.x + (size_t)win * XSTRIDE, g_norm, b.win[win].use_leg);
    }
    imu_stage(rs, lane, r);
  }
  lds_barrier();
  const unsigned long long livem = __ballot(live), badm = __ballot(bad);
  const int row = min(lane, 30);
  for (int fl = 0; fl < 64; ++fl) {
    if (f0 + fl >= NF) break;
    double u = 0.0;
    if ((livem >> fl) & 1ULL) {
      double uq[31];
      imu_info_row(b.prep[f0 + fl].sqrt_info, row, uq);
      u = imu_row_dot(uq, rs, fl);
    }
    const bool nan_f = (badm >> fl) & 1ULL;
    if (res_out && lane < 31) res_out[(size_t)(f0 + fl) * 31 + lane] = nan_f ? NAN : u;
    const double c = wave_sum(lane < 31 ? u * u : 0.0);
    if (lane == 0) rs[31 * 64 + fl] = nan_f ? NAN : 0.5 * c;
  }
  lds_barrier();
  if (f < NF) cost_out[f] = rs[31 * 64 + lane];
}

// one workgroup of 128 threads per window
__global__ void __launch_bounds__(128) k_resid_window(BatchDev b, ResidLm lm, const double *imu_cost, vilo_window_residual *out) {
  using namespace vilo;
  __shared__ double red[128];
  __shared__ double dxs[VILO_MAX_PRIOR_DIM];
  __shared__ int ired[8];
  const int win = blockIdx.x, tid = threadIdx.x;
  const WinMeta wm = b.win[win];
  // prior: 1/2 (dx^T (H dx + 2 b0) + c0) at x, from cost_eval.hpp's prior pieces
  double pri = 0.0;
  if (wm.prior_n > 0) {
    const int n = wm.prior_n;
    if (tid < wm.prior_nb) prior_dx_block(b, win, tid, b.x + (size_t)win * XSTRIDE, dxs);
    __syncthreads();
    const double *Hp = b.prior_H + (size_t)win * 96 * 96, *b0 = b.prior_b0 + (size_t)win * 96;
    if (tid < n) {
      double sacc = 0.0;
      for (int q = 0; q < n; ++q) sacc += Hp[(size_t)q * n + tid] * dxs[q];
      pri = prior_row_term(dxs[tid], sacc, b0[tid]);
    }
  }
  // landmark sums in caller order: thread t takes l = t, t + 128, ...; one fixed tree over the threads
  double vis = 0.0, pl = 0.0;
  int nb = 0, nh = 0, nout = 0, nneg = 0;
  for (int l = tid; l < wm.L; l += 128) {
    const int o = wm.lm_off + l;
    vis += lm.cost[o];
    pl += lm.plain[o];
    nb += lm.nb[o];
    nh += lm.nh[o];
    nout += lm.flags[o] & 1;
    nneg += (lm.flags[o] >> 1) & 1;
  }
  block_sum128x3(pri, vis, pl, red);
  // (integer counts: exact in any order)
  nb = wave_sum_int(nb); nh = wave_sum_int(nh); nout = wave_sum_int(nout); nneg = wave_sum_int(nneg);
  if ((tid & 63) == 0) { ired[4 * (tid >> 6) + 0] = nb; ired[4 * (tid >> 6) + 1] = nh; ired[4 * (tid >> 6) + 2] = nout; ired[4 * (tid >> 6) + 3] = nneg; }
  __syncthreads();
  if (tid == 0) {
    vilo_window_residual r;
    r.prior_cost = wm.prior_n > 0 ? 0.5 * (pri + b.prior_c0[win]) : 0.0;
    double cost = r.prior_cost;
    int status = 0;
    for (int k = 0; k < 10; ++k) {
      const double c = imu_cost[(size_t)win * 10 + k];
      r.imu_cost[k] = c;
      cost += c;
      if (isnan(c)) status = 2;
    }
    r.visual_cost = vis;
    r.visual_cost_plain = pl;
    r.cost = cost + vis;
    r.n_visual_blocks = ired[0] + ired[4];
    r.n_huber_active = ired[1] + ired[5];
    r.n_outliers = ired[2] + ired[6];
    r.n_negative_depth = ired[3] + ired[7];
    r.status = status;
    r.pad = 0;
    out[win] = r;
  }
}

int vilo_resid_landmark_flags_launch(vilo_ctx *ctx, const BatchDev &b, double threshold_px, double *scratch_d3, int *scratch_i2, unsigned char *flags) {
  if (b.n_waves <= 0) return VILO_OK;
  ResidLm lm;
  lm.cost = scratch_d3; lm.reproj = scratch_d3 + b.n_lm; lm.plain = scratch_d3 + 2 * (size_t)b.n_lm;
  lm.nb = scratch_i2; lm.nh = scratch_i2 + b.n_lm; lm.flags = flags;
  hipLaunchKernelGGL(k_resid_landmarks, dim3(b.n_waves), dim3(64), 0, ctx->stream, b, ctx->cfg.focal_length / 1.5, ctx->cfg.huber_delta, ctx->cfg.focal_length, threshold_px,
                     (const int *)nullptr, lm, (double *)nullptr);
  VILO_HIP(hipGetLastError());
  return VILO_OK;
}

extern "C" void vilo_default_residual_opts(vilo_residual_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->outlier_threshold_px = 3.0;
}

extern "C" int vilo_batch_residuals(vilo_ctx *ctx, vilo_batch *bt, const vilo_residual_opts *opts, vilo_window_residual *windows, double *lm_cost,
                                    double *lm_reproj_px, uint8_t *lm_flags, double *obs_residuals, double *imu_residuals) {
  if (!ctx || !bt || !windows) return VILO_ERR_BAD_ARG;
  if (bt->mask.stale(ctx, "vilo_batch_residuals") != VILO_OK) return VILO_ERR_HIP;
  vilo_residual_opts o;
  if (opts) o = *opts; else vilo_default_residual_opts(&o);
  if (!isfinite(o.outlier_threshold_px) || !(o.outlier_threshold_px >= 0.0)) {
    ctx->err = "vilo_batch_residuals: outlier_threshold_px must be finite and >= 0";
    return VILO_ERR_BAD_ARG;
  }
  VILO_HIP(hipSetDevice(ctx->device));
  const BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm, NF = W * 10;
  const int *obs_row = nullptr;
  const int n_rows = bt->lm.n_obs_rows;
  const int rc = bt->lm.obs_rows(ctx, bt->arena, &obs_row);   // (batch data, uploaded at the first call: before the scope opens)
  if (rc != VILO_OK) return rc;
  BatchCall call(ctx, bt, &vilo_ctx::last_resid_ms);
  // the call's device memory: window records | per-landmark values | interval costs, residuals | observation residuals | re-integration copies
  const size_t o_win = call.lay.take<vilo_window_residual>(W);
  const size_t o_lc = call.lay.take<double>(n_lm), o_lr = call.lay.take<double>(n_lm), o_lp = call.lay.take<double>(n_lm);
  const size_t o_nb = call.lay.take<int>(n_lm), o_nh = call.lay.take<int>(n_lm), o_fl = call.lay.take<unsigned char>(n_lm);
  const size_t o_ic = call.lay.take<double>(NF), o_ir = call.lay.take<double>(31 * (size_t)NF, imu_residuals != nullptr);
  const size_t o_or = call.lay.take<double>(4 * (size_t)n_rows, obs_residuals != nullptr);
  const ReintegrationBlocks rp(call.lay, bd, 2);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  ResidLm lm;
  lm.cost = call.ptr<double>(o_lc); lm.reproj = call.ptr<double>(o_lr); lm.plain = call.ptr<double>(o_lp);
  lm.nb = call.ptr<int>(o_nb); lm.nh = call.ptr<int>(o_nh); lm.flags = call.ptr<unsigned char>(o_fl);
  double *d_ic = call.ptr<double>(o_ic), *d_ir = imu_residuals ? call.ptr<double>(o_ir) : nullptr, *d_or = obs_residuals ? call.ptr<double>(o_or) : nullptr;
  const double sq = ctx->cfg.focal_length / 1.5, ha = ctx->cfg.huber_delta, gn = ctx->cfg.g_norm;
  VILO_HIP(call.start());
  // a masked landmark (vilo_batch_mask_landmarks) has no valid observation: k_resid_landmarks writes none of its rows, which come back NaN
  if (d_or && bt->mask.n_masked > 0) VILO_HIP(hipMemsetAsync(d_or, 0xFF, sizeof(double) * 4 * (size_t)n_rows, ctx->stream));
  BatchDev b = bd;
  if (call.reintegrate(b, rp) != VILO_OK) return VILO_ERR_HIP;
  if (bd.n_waves > 0)
    hipLaunchKernelGGL(k_resid_landmarks, dim3(bd.n_waves), dim3(64), 0, ctx->stream, b, sq, ha, ctx->cfg.focal_length, o.outlier_threshold_px, obs_row,
                       lm, d_or);
  hipLaunchKernelGGL(k_resid_imu, dim3((NF + 63) / 64), dim3(64), 0, ctx->stream, b, gn, d_ic, d_ir);
  hipLaunchKernelGGL(k_resid_window, dim3(W), dim3(128), 0, ctx->stream, b, lm, (const double *)d_ic, call.ptr<vilo_window_residual>(o_win));
  VILO_HIP(call.finish());
  VILO_HIP(call.down(windows, call.ptr<char>(o_win), sizeof(vilo_window_residual) * (size_t)W));
  VILO_HIP(call.down(lm_cost, lm.cost, sizeof(double) * (size_t)n_lm));
  VILO_HIP(call.down(lm_reproj_px, lm.reproj, sizeof(double) * (size_t)n_lm));
  VILO_HIP(call.down(lm_flags, lm.flags, (size_t)n_lm));
  VILO_HIP(call.down(obs_residuals, d_or, sizeof(double) * 4 * (size_t)n_rows));
  VILO_HIP(call.down(imu_residuals, d_ir, sizeof(double) * 31 * (size_t)NF));
  return VILO_OK;
}

extern "C" int vilo_window_residuals(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                     const vilo_residual_opts *opts, vilo_window_residual *windows, double *lm_cost, double *lm_reproj_px,
                                     uint8_t *lm_flags, double *obs_residuals, double *imu_residuals) {
  if (!ctx || n_windows < 1 || !in || !state || !windows) return VILO_ERR_BAD_ARG;
  if (opts && (!isfinite(opts->outlier_threshold_px) || !(opts->outlier_threshold_px >= 0.0))) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_residuals(ctx, bt, opts, windows, lm_cost, lm_reproj_px, lm_flags, obs_residuals, imu_residuals);
  });
}

extern "C" double vilo_last_residuals_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_resid_ms : -1.0; }
