// The cost of every window of a batch at up to 16 trial steps from its current device state, the state left where it is
// (vilo_batch_trial_cost, include/vilo_gpu.h; TrustRegionMinimizer's candidate evaluation, which the solver runs on xc, opened to a
// caller's own steps). The cost's arithmetic is cost_eval.hpp's pieces, as in the solver's cost kernels and in kernels_resid.hip.
//
// Four launches, one code path for every batch size and every K; no atomics, every sum in a fixed order. The call evaluates K + 1 columns
// per window: the K trial states and, as column K, the state itself (the base cost every cost_change needs), all by the same arithmetic.
//   k_trial_states     one wave per (window, column): x [+] alpha * delta into the call's scratch through retract_step.hpp, the device
//                      function k_retract runs; the NUMERIC decision and the negative-depth count per column. Column K, and a NUMERIC
//                      column, is a plain copy of x and lambda.
//   k_trial_landmarks  one wave per packed visual wave, lane = landmark, walking the wave's frames. The columns' frame poses, extrinsics
//                      and td (92 doubles each) are staged in LDS with the lanes' inverse depths and cost accumulators. t is the outer
//                      loop: a wave's observation and flag rows are fetched once per t and used for every column before the next t.
//   k_trial_imu        lane = factor for the raw residual, then lane = row of sqrt_info, the columns in chunks of TI_KC: a row
//                      (imu_info_row) is loaded once per chunk and applied to the chunk's residual vectors (imu_row_dot).
//   k_trial_window     one workgroup per window: the prior's cost at every column with prior_H read once (H dx_k for all k per row), the
//                      landmark and interval sums in k_resid_window's stride, tree and order, the records and `best`.
// The walk keeps nothing per column in registers: per (t, column) it forms the landmark's start-frame point and world point again from the
// staged column (two quaternion rotations more per block than a one-state walk, which forms them once per landmark) and adds into an LDS accumulator.
// Holding them would take 6 doubles per column and lane, 192 registers at 16 columns, and a register array indexed by a run-time column
// lives in scratch; DESIGN 4.30 has the figures.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "accept_body.hpp"
#include "batch_call.hpp"
#include "lin_common.hpp"
#include "retract_step.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_trial_record) == 48, "vilo_trial_record: 48 bytes (include/vilo_gpu.h)");

#define TR_MAXC (VILO_TRIAL_MAX_STEPS + 1)   // columns of a call: the steps and the base
#define TL_XS 96                             // a staged column: poses at 7 k, extrinsics at TL_EX, td at TL_TD
#define TL_EX 80
#define TL_TD 94
#define TL_COL (TL_XS + 64 + 64)             // + the lanes' inverse depths and cost accumulators
#define TI_KC 4                              // columns of k_trial_imu's chunk: 4 x 16 KB of LDS, two workgroups per CU

struct TrialArgs {
  int K;                       // steps per window; the columns are K + 1
  const double *state_step;    // [W][K][RT_STATE], or null
  const double *lm_step;       // [K sum L] (vilo_batch_hessian_vector's layout), or null
  const double *alpha;         // [W][K], or null
  const unsigned char *mask;   // [n_lm] device order: the landmark mask in force, or null
  double *xt;                  // [W][K + 1][XSTRIDE] the columns' states
  double *lamt;                // [K + 1][n_lm] their inverse depths, device order
  int *numeric, *nneg;         // [W][K + 1]
  double *lc;                  // [K + 1][n_lm] visual cost per landmark, caller order
  double *ic;                  // [K + 1][W * 10] cost per interval
};

__global__ void __launch_bounds__(64) k_trial_states(BatchDev b, TrialArgs a) {
  const int win = blockIdx.x, k = blockIdx.y, lane = threadIdx.x, K = a.K, KK = K + 1;
  const WinMeta wm = b.win[win];
  const bool base = k == K;
  StepView v;
  v.step = (a.state_step && !base) ? a.state_step + ((size_t)win * K + k) * RT_STATE : nullptr;
  v.lm_step = (a.lm_step && !base) ? a.lm_step + (size_t)K * wm.lm_off + (size_t)k * wm.L : nullptr;
  v.mask = a.mask;
  v.perm = b.lm_perm;
  v.al = (a.alpha && !base) ? a.alpha[(size_t)win * K + k] : 1.0;
  bool numeric = false;
  if (!base) {
    const StepStats st = rt_scan(wm, v, lane);
    numeric = __any(st.bad);
  }
  double *xo = a.xt + ((size_t)win * KK + k) * XSTRIDE, *lo = a.lamt + (size_t)k * b.n_lm + wm.lm_off;
  rt_store(wm, v, lane, b.x + (size_t)win * XSTRIDE, b.lam + wm.lm_off, xo, lo, !base && !numeric, true);
  // (a lane reads back only what it stored itself)
  int nneg = 0;
  for (int l = lane; l < wm.L; l += 64)
    if (!(a.mask && a.mask[wm.lm_off + l]) && lo[l] < 0.0) ++nneg;
  nneg = wave_sum_int(nneg);
  if (lane == 0) {
    a.numeric[(size_t)win * KK + k] = numeric ? 1 : 0;
    a.nneg[(size_t)win * KK + k] = numeric ? 0 : nneg;
  }
}

__global__ void __launch_bounds__(64) k_trial_landmarks(BatchDev b, TrialArgs a, double sq, double huber_a) {
  using namespace vilo;
  extern __shared__ double tl_lds[];   // [K + 1][TL_COL]
  const int KK = a.K + 1;
  const WaveMeta wv = b.wave[blockIdx.x];
  const WinMeta wm = b.win[wv.win];
  const int lane = threadIdx.x;
  int cs[4], cn[4], ckm[4], cgo[4];
  const LaneSeg ls = lane_segment(wv, b.chunk, lane, cs, cn, ckm, cgo);
  const double *xw = a.xt + (size_t)wv.win * KK * XSTRIDE;
  for (int e = lane; e < KK * TL_XS; e += 64) {
    const int k = e / TL_XS, i = e - k * TL_XS;
    const int src = i < 7 * VILO_MAX_FRAMES ? XO_POSE + i : (i >= TL_EX && i < TL_EX + 14) ? XO_EX + (i - TL_EX) : i == TL_TD ? XO_TD : -1;
    if (src >= 0) tl_lds[k * TL_COL + i] = xw[(size_t)k * XSTRIDE + src];
  }
  for (int k = 0; k < KK; ++k) {
    tl_lds[k * TL_COL + TL_XS + lane] = ls.active ? a.lamt[(size_t)k * b.n_lm + ls.gi] : 1.0;
    tl_lds[k * TL_COL + TL_XS + 64 + lane] = 0.0;
  }
  lds_barrier();
  if (!ls.active) return;
  const int n = wv.n_lanes, s = ls.s;
  const double *obs = b.obs + wv.obs_off;
  const unsigned char *flg = b.flags + wv.flag_off;
  auto row = [&](int t, int r) { return obs_at(obs, n, lane, t, r); };
  // the start frame's row, read once
  const double u0 = row(0, OBS_LX), u1 = row(0, OBS_LY), u2 = row(0, OBS_LZ), v0 = row(0, OBS_LVX), v1 = row(0, OBS_LVY), t0 = row(0, OBS_TD);
  for (int t = 0; t < wv.kmax; ++t) {
    const unsigned char fl = flg[(size_t)t * n + lane];
    if (!(fl & 1)) continue;
    // this frame's row, read once for every column
    const double tj = row(t, OBS_TD);
    double lx = 0.0, ly = 0.0, lvx = 0.0, lvy = 0.0, rx = 0.0, ry = 0.0, rvx = 0.0, rvy = 0.0;
    if (t > 0) { lx = row(t, OBS_LX); ly = row(t, OBS_LY); lvx = row(t, OBS_LVX); lvy = row(t, OBS_LVY); }
    if (fl & 2) { rx = row(t, OBS_RX); ry = row(t, OBS_RY); rvx = row(t, OBS_RVX); rvy = row(t, OBS_RVY); }
    const int fj = min(s + t, VILO_MAX_FRAMES - 1);
    for (int k = 0; k < KK; ++k) {
      const double *xk = tl_lds + k * TL_COL;
      // the factors' form (cost_eval.hpp) on the staged column: the start-frame point and, for t > 0, its world point, once per (t, column)
      const double td = xk[TL_TD];
      const double *ex0 = xk + TL_EX, *ex1 = xk + TL_EX + 7;
      const quat qic = ldq_pose(ex0);
      const v3 tic = ld3(ex0);
      const v3 p_i = start_point(u0, u1, u2, v0, v1, t0, td, 1.0 / xk[TL_XS + lane], qic, tic);
      const double dtj = td - tj;
      double cost = xk[TL_XS + 64 + lane];
      v3 p_j = p_i;
      if (t > 0) {
        p_j = frame_point(xk + 7 * fj, world_point(xk + 7 * s, p_i));
        cost += camera_block(camera_point(qic, tic, p_j), lx - lvx * dtj, ly - lvy * dtj, sq, huber_a).rho0;
      }
      if (fl & 2) cost += camera_block(camera_point(ldq_pose(ex1), ld3(ex1), p_j), rx - rvx * dtj, ry - rvy * dtj, sq, huber_a).rho0;
      tl_lds[k * TL_COL + TL_XS + 64 + lane] = cost;
    }
  }
  const int o = wm.lm_off + b.lm_perm[ls.gi];
  for (int k = 0; k < KK; ++k) a.lc[(size_t)k * b.n_lm + o] = 0.5 * tl_lds[k * TL_COL + TL_XS + 64 + lane];
}

// one wave per 64 factors
__global__ void __launch_bounds__(64) k_trial_imu(BatchDev b, TrialArgs a, double g_norm) {
  using namespace vilo;
  extern __shared__ double ti_lds[];   // [chunk column][entry][factor of the wave]; row 31: 1/2 |u|^2 per factor
  const int KK = a.K + 1;
  const int lane = threadIdx.x, f0 = blockIdx.x * 64, f = f0 + lane;
  const int NF = b.W * 10;
  const int win = f / 10;
  const bool live = f < NF && !b.imu_skip[f];
  const bool bad = live && b.prep_bad && b.prep_bad[f];
  const bool leg = live && b.win[win].use_leg;
  const unsigned long long livem = __ballot(live), badm = __ballot(bad);
  const int row = min(lane, 30);
  for (int k0 = 0; k0 < KK; k0 += TI_KC) {
    const int nk = min(TI_KC, KK - k0);
    for (int kc = 0; kc < nk; ++kc) {
      ImuResid r = {};
      if (live) r = imu_factor_raw(b, f, a.xt + ((size_t)win * KK + k0 + kc) * XSTRIDE, g_norm, leg);
      imu_stage(ti_lds + kc * 32 * 64, lane, r);
    }
    lds_barrier();
    for (int fl = 0; fl < 64; ++fl) {
      if (f0 + fl >= NF) break;
      if (!((livem >> fl) & 1ULL)) continue;   // (its costs stay 0)
      double uq[31];
      imu_info_row(b.prep[f0 + fl].sqrt_info, row, uq);
      const bool nan_f = (badm >> fl) & 1ULL;
      for (int kc = 0; kc < nk; ++kc) {
        double *rs = ti_lds + kc * 32 * 64;
        const double u = imu_row_dot(uq, rs, fl);
        const double c = wave_sum(lane < 31 ? u * u : 0.0);
        if (lane == 0) rs[31 * 64 + fl] = nan_f ? NAN : 0.5 * c;
      }
    }
    lds_barrier();
    if (f < NF)
      for (int kc = 0; kc < nk; ++kc) a.ic[(size_t)(k0 + kc) * NF + f] = ti_lds[kc * 32 * 64 + 31 * 64 + lane];
    lds_barrier();
  }
}

// one workgroup of 128 threads per window
__global__ void __launch_bounds__(128) k_trial_window(BatchDev b, TrialArgs a, vilo_trial_record *base, vilo_trial_record *rec, int *best) {
  using namespace vilo;
  __shared__ double red[8];
  __shared__ double dxs[TR_MAXC * VILO_MAX_PRIOR_DIM];   // dx of every column; then a thread's term of the prior's sum in place
  __shared__ double pris[TR_MAXC], viss[TR_MAXC], costs[TR_MAXC], ccs[TR_MAXC];
  __shared__ int stats[TR_MAXC];
  const int win = blockIdx.x, tid = threadIdx.x, K = a.K, KK = K + 1;
  const WinMeta wm = b.win[win];
  const int n = wm.prior_n;
  // prior: 1/2 (dx^T (H dx + 2 b0) + c0) at every column (cost_eval.hpp's prior pieces); a row of prior_H is read once for all columns
  if (n > 0) {
    if (tid < wm.prior_nb)
      for (int k = 0; k < KK; ++k) prior_dx_block(b, win, tid, a.xt + ((size_t)win * KK + k) * XSTRIDE, dxs + k * VILO_MAX_PRIOR_DIM);
    __syncthreads();
    const double *Hp = b.prior_H + (size_t)win * 96 * 96, *b0 = b.prior_b0 + (size_t)win * 96;
    double sacc[TR_MAXC];
#pragma unroll
    for (int k = 0; k < TR_MAXC; ++k) sacc[k] = 0.0;
    if (tid < n)
      for (int q = 0; q < n; ++q) {
        const double h = Hp[(size_t)q * n + tid];
#pragma unroll
        for (int k = 0; k < TR_MAXC; ++k)
          if (k < KK) sacc[k] += h * dxs[k * VILO_MAX_PRIOR_DIM + q];
      }
    __syncthreads();
    if (tid < n) {
      const double b0r = b0[tid];
#pragma unroll
      for (int k = 0; k < TR_MAXC; ++k)
        if (k < KK) dxs[k * VILO_MAX_PRIOR_DIM + tid] = prior_row_term(dxs[k * VILO_MAX_PRIOR_DIM + tid], sacc[k], b0r);
    }
    __syncthreads();
  }
  // per column: the prior's terms and the landmark costs in caller order (thread t takes l = t, t + 128, ...), one fixed tree
  for (int k = 0; k < KK; ++k) {
    double pri = (n > 0 && tid < n) ? dxs[k * VILO_MAX_PRIOR_DIM + tid] : 0.0, vis = 0.0, z = 0.0;
    const double *lck = a.lc + (size_t)k * b.n_lm + wm.lm_off;
    for (int l = tid; l < wm.L; l += 128) vis += lck[l];
    block_sum128x3(pri, vis, z, red);
    if (tid == 0) { pris[k] = pri; viss[k] = vis; }
  }
  __syncthreads();
  bool invalid = false;
  if (b.prep_bad)
    for (int j = 0; j < 10; ++j) invalid |= !b.imu_skip[win * 10 + j] && b.prep_bad[win * 10 + j];
  vilo_trial_record r;
  const bool numeric = tid < KK && a.numeric[(size_t)win * KK + tid];
  if (tid < KK) {
    const int NF = b.W * 10;
    r.prior_cost = n > 0 ? 0.5 * (pris[tid] + b.prior_c0[win]) : 0.0;
    double cost = r.prior_cost, imu = 0.0;
    for (int j = 0; j < 10; ++j) {
      const double c = a.ic[(size_t)tid * NF + win * 10 + j];
      imu += c;
      cost += c;
    }
    r.imu_cost = imu;
    r.visual_cost = viss[tid];
    r.cost = cost + viss[tid];
    r.n_negative_depth = a.nneg[(size_t)win * KK + tid];
    r.status = numeric ? VILO_TRIAL_NUMERIC : invalid ? VILO_TRIAL_INVALID : !isfinite(r.cost) ? VILO_TRIAL_NOT_FINITE : VILO_TRIAL_OK;
    costs[tid] = r.cost;
    stats[tid] = r.status;
  }
  __syncthreads();
  if (tid < K) {
    r.cost_change = costs[K] - r.cost;
    if (numeric) { r.cost = NAN; r.visual_cost = NAN; r.imu_cost = NAN; r.prior_cost = NAN; r.cost_change = NAN; }
    rec[(size_t)win * K + tid] = r;
    ccs[tid] = r.cost_change;
  } else if (tid == K && base) {
    r.cost_change = 0.0;
    base[win] = r;
  }
  __syncthreads();
  if (tid == 0 && best) {
    // the smallest k of status OK with the lowest cost among those that lower the cost
    int bk = -1;
    double bc = 0.0;
    for (int k = 0; k < K; ++k)
      if (stats[k] == VILO_TRIAL_OK && ccs[k] > 0.0 && (bk < 0 || costs[k] < bc)) { bk = k; bc = costs[k]; }
    best[win] = bk;
  }
}

extern "C" double vilo_last_trial_cost_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_trial_ms : -1.0; }

extern "C" int vilo_batch_trial_cost(vilo_ctx *ctx, vilo_batch *bt, int n_steps, const double *state_step, const double *lm_step, const double *alpha,
                                     vilo_trial_record *base, vilo_trial_record *records, int32_t *best) {
  if (!ctx || !bt || !records) return VILO_ERR_BAD_ARG;
  if (n_steps < 1 || n_steps > VILO_TRIAL_MAX_STEPS) {
    ctx->err = "vilo_batch_trial_cost: 1 <= n_steps <= VILO_TRIAL_MAX_STEPS (16) is required";
    return VILO_ERR_BAD_ARG;
  }
  const BatchDev &bd = bt->d;
  if (bd.rp_on) {
    ctx->err = "vilo_batch_trial_cost: vilo_batch_set_samples is in force on this batch: every trial state would need its own re-integration, which this call does not do (switch it off first)";
    return VILO_ERR_UNSUPPORTED;
  }
  if (bt->mask.stale(ctx, "vilo_batch_trial_cost") != VILO_OK) return VILO_ERR_HIP;
  const int W = bd.W, K = n_steps, KK = K + 1, NF = W * 10;
  const size_t n_lm = (size_t)std::max(bd.n_lm, 0);
  BatchCall call(ctx, bt, &vilo_ctx::last_trial_ms);
  // the call's device memory: state steps | landmark steps | step lengths | the columns' states, inverse depths, decisions | landmark and
  // interval costs | records
  const size_t o_s = call.lay.take<double>(RT_STATE * (size_t)W * K, state_step != nullptr), o_l = call.lay.take<double>(K * n_lm, lm_step != nullptr && n_lm > 0),
               o_a = call.lay.take<double>((size_t)W * K, alpha != nullptr);
  const size_t o_xt = call.lay.take<double>((size_t)W * KK * XSTRIDE), o_lt = call.lay.take<double>(KK * n_lm, n_lm > 0);
  const size_t o_nu = call.lay.take<int>((size_t)W * KK), o_nn = call.lay.take<int>((size_t)W * KK);
  const size_t o_lc = call.lay.take<double>(KK * n_lm, n_lm > 0), o_ic = call.lay.take<double>((size_t)KK * NF);
  const size_t o_b = call.lay.take<vilo_trial_record>(W, base != nullptr), o_r = call.lay.take<vilo_trial_record>((size_t)W * K), o_best = call.lay.take<int>(W, best != nullptr);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  TrialArgs a;
  a.K = K;
  a.state_step = state_step ? call.ptr<double>(o_s) : nullptr;
  a.lm_step = lm_step && n_lm > 0 ? call.ptr<double>(o_l) : nullptr;
  a.alpha = alpha ? call.ptr<double>(o_a) : nullptr;
  a.mask = bt->mask.d_mask;
  a.xt = call.ptr<double>(o_xt); a.lamt = call.ptr<double>(o_lt);
  a.numeric = call.ptr<int>(o_nu); a.nneg = call.ptr<int>(o_nn);
  a.lc = call.ptr<double>(o_lc); a.ic = call.ptr<double>(o_ic);
  // (not timed)
  if (a.state_step) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_s), state_step, sizeof(double) * RT_STATE * (size_t)W * K, hipMemcpyHostToDevice, ctx->stream));
  if (a.lm_step) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_l), lm_step, sizeof(double) * K * n_lm, hipMemcpyHostToDevice, ctx->stream));
  if (a.alpha) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_a), alpha, sizeof(double) * (size_t)W * K, hipMemcpyHostToDevice, ctx->stream));
  if (!ctx->trial_attr_set) {
    VILO_HIP(hipFuncSetAttribute((const void *)k_trial_imu, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * 32 * 64 * TI_KC)));
    ctx->trial_attr_set = true;
  }
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_trial_states, dim3(W, KK), dim3(64), 0, ctx->stream, bd, a);
  if (bd.n_waves > 0)
    hipLaunchKernelGGL(k_trial_landmarks, dim3(bd.n_waves), dim3(64), sizeof(double) * TL_COL * KK, ctx->stream, bd, a, ctx->cfg.focal_length / 1.5, ctx->cfg.huber_delta);
  hipLaunchKernelGGL(k_trial_imu, dim3((NF + 63) / 64), dim3(64), sizeof(double) * 32 * 64 * std::min(KK, TI_KC), ctx->stream, bd, a, ctx->cfg.g_norm);
  hipLaunchKernelGGL(k_trial_window, dim3(W), dim3(128), 0, ctx->stream, bd, a, base ? call.ptr<vilo_trial_record>(o_b) : (vilo_trial_record *)nullptr,
                     call.ptr<vilo_trial_record>(o_r), best ? call.ptr<int>(o_best) : (int *)nullptr);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(records, call.ptr<char>(o_r), sizeof(vilo_trial_record) * (size_t)W * K));
  VILO_HIP(call.down(base, call.ptr<char>(o_b), sizeof(vilo_trial_record) * (size_t)W));
  VILO_HIP(call.down(best, call.ptr<char>(o_best), sizeof(int32_t) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_trial_cost(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, int n_steps,
                                      const double *state_step, const double *lm_step, const double *alpha, vilo_trial_record *base,
                                      vilo_trial_record *records, int32_t *best) {
  if (!ctx || n_windows < 1 || !in || !state || !records) return VILO_ERR_BAD_ARG;
  if (n_steps < 1 || n_steps > VILO_TRIAL_MAX_STEPS) {
    ctx->err = "vilo_window_trial_cost: 1 <= n_steps <= VILO_TRIAL_MAX_STEPS (16) is required";
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state,
                         [&](vilo_batch *bt) { return vilo_batch_trial_cost(ctx, bt, n_steps, state_step, lm_step, alpha, base, records, best); });
}
