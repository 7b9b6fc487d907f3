// Cost gradient and Gauss-Newton diagonal of every window of a batch at its current device state (vilo_batch_gradient, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0), exactly as vilo_batch_covariance runs it: the windows'
// SolverStates are copied aside before and back after; x, lambda and the prior are only read. No factor is evaluated here: J^T r and
// diag(J^T J) are in what that pass leaves — the r column and the diagonal of the 23-column visual Gram slots and of the 39 x 39 IMU
// Grams, lm_gbuf[0] / lm_E for the inverse depths — and in the prior's H, b0 and H dx.
//
// k_gradient, one workgroup per window, one code path for every batch size, all FP64:
//   1. owner-computes: thread d < 222 owns output dimension d of the caller's layout (caller_cd, gn_system.hpp) and walks its
//      contributions in one fixed order (state_entry_gh, gn_system.hpp: visual Gram slots, the two IMU Grams, the prior) with plain adds
//      in a register. No floating-point atomics; nothing depends on the batch a window shares or on its position.
//   2. the landmarks' lm_g / lm_E go to the caller's order (lm_off + lm_perm).
//   3. the window record: thread t takes entries t, t + 256, ... of the list [222 state entries | the landmarks in caller order], then one
//      fixed halving tree over the threads (sum of squares, max |g| with its position — ties to the lower position —, max |g| / sqrt(h),
//      the count of free coordinates, a not-finite flag).
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "gn_system.hpp"

static_assert(sizeof(vilo_window_gradient_record) == 48, "vilo_window_gradient_record: 48 bytes (include/vilo_gpu.h)");

// a candidate of the record's tree: position p of the list is free, with gradient g and diagonal h
struct GradPart {
  double sq, mx, sc;
  int pos, nfree, bad;
};
__device__ __forceinline__ void grad_take(GradPart &a, int p, double g, double h) {
  const double ag = fabs(g);
  a.sq += g * g;
  if (ag > a.mx) { a.mx = ag; a.pos = p; }   // (entries come in ascending position: a tie keeps the lower one)
  if (h > 0.0) a.sc = fmax(a.sc, ag / sqrt(h));
  ++a.nfree;
  if (!isfinite(g) || !isfinite(h)) a.bad = 1;
}

__global__ void __launch_bounds__(GN_T) k_gradient(BatchDev b, vilo_window_gradient_record *rec, double *sg_out, double *sd_out, double *lg_out,
                                                  double *ld_out) {
  using namespace vilo;
  __shared__ double dxs[VILO_MAX_PRIOR_DIM];
  __shared__ short inv_pmap[CD_N];
  __shared__ double r_sq[GN_T], r_mx[GN_T], r_sc[GN_T];
  __shared__ int r_pos[GN_T], r_nf[GN_T], r_bad[GN_T];
  const int win = blockIdx.x, tid = threadIdx.x;
  const WinMeta wm = b.win[win];
  const int F = wm.n_frames, L = wm.L;
  double *sg = sg_out + (size_t)win * GN_NS, *sd = sd_out + (size_t)win * GN_NS;
  double *lg = lg_out + wm.lm_off, *ld = ld_out + wm.lm_off;
  if (b.win_bad && b.win_bad[win]) {   // a preintegration covariance without sqrt_info: the window is not linearised (k_init_state marks it done)
    for (int e = tid; e < GN_NS; e += GN_T) { sg[e] = NAN; sd[e] = NAN; }
    for (int l = tid; l < L; l += GN_T) { lg[l] = NAN; ld[l] = NAN; }
    if (tid == 0) {
      vilo_window_gradient_record r;
      r.max_norm = NAN; r.norm = NAN; r.scaled_max = NAN;
      r.argmax_kind = -1; r.argmax_index = -1; r.argmax_component = -1;
      r.n_free = 0; r.status = 2; r.pad = 0;
      rec[win] = r;
    }
    return;
  }
  prior_view_init(b, wm, win, b.prior_map + (size_t)win * 96, dxs, inv_pmap);

  // ---- 1. the 222 state entries ----
  double g = 0.0, h = 0.0;
  bool act = false;
  if (tid < GN_NS) {
    const int cd = caller_cd(tid);
    act = cd_active(cd, F, wm.const_mask);
    if (act) state_entry_gh<true>(b, wm, win, cd, inv_pmap, dxs, g, h);
    sg[tid] = g;
    sd[tid] = h;
  }
  // ---- 2. landmarks to the caller's order ----
  {
    const double *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
    const int *perm = b.lm_perm + wm.lm_off;
    for (int l = tid; l < L; l += GN_T) {
      const int o = perm[l];
      lg[o] = lmg[l];
      ld[o] = lmE[l];
    }
  }
  __syncthreads();   // (the landmark values are read back in caller order below)

  // ---- 3. the window record ----
  GradPart p;
  p.sq = 0.0; p.mx = -1.0; p.sc = 0.0; p.pos = -1; p.nfree = 0; p.bad = 0;
  if (act) grad_take(p, tid, g, h);
  for (int e = tid; e < L; e += GN_T) grad_take(p, GN_NS + e, lg[e], ld[e]);   // (positions tid + 256 m ascend with m: GN_NS + e > tid)
  r_sq[tid] = p.sq; r_mx[tid] = p.mx; r_sc[tid] = p.sc; r_pos[tid] = p.pos; r_nf[tid] = p.nfree; r_bad[tid] = p.bad;
  __syncthreads();
  for (int st = GN_T / 2; st > 0; st >>= 1) {
    if (tid < st) {
      const int o = tid + st;
      r_sq[tid] += r_sq[o];
      r_sc[tid] = fmax(r_sc[tid], r_sc[o]);
      r_nf[tid] += r_nf[o];
      r_bad[tid] |= r_bad[o];
      const bool take = r_mx[o] > r_mx[tid] || (r_mx[o] == r_mx[tid] && r_pos[o] >= 0 && (r_pos[tid] < 0 || r_pos[o] < r_pos[tid]));
      if (take) { r_mx[tid] = r_mx[o]; r_pos[tid] = r_pos[o]; }
    }
    __syncthreads();
  }
  if (tid == 0) {
    vilo_window_gradient_record r;
    const int pos = r_pos[0], bad = r_bad[0];
    r.max_norm = bad ? NAN : (pos >= 0 ? r_mx[0] : 0.0);
    r.norm = bad ? NAN : sqrt(r_sq[0]);
    r.scaled_max = bad ? NAN : r_sc[0];
    int kind = -1, idx = -1, comp = -1;
    if (!bad && pos >= 0) {
      if (pos < 66) { kind = VILO_BLK_POSE; idx = pos / 6; comp = pos % 6; }
      else if (pos < 165) { kind = VILO_BLK_SB; idx = (pos - 66) / 9; comp = (pos - 66) % 9; }
      else if (pos < 209) { kind = VILO_BLK_LB; idx = (pos - 165) / 4; comp = (pos - 165) % 4; }
      else if (pos < 221) { kind = VILO_BLK_EX; idx = (pos - 209) / 6; comp = (pos - 209) % 6; }
      else if (pos == 221) { kind = VILO_BLK_TD; idx = 0; comp = 0; }
      else { kind = VILO_BLK_FEAT; idx = pos - GN_NS; comp = 0; }
    }
    r.argmax_kind = kind; r.argmax_index = idx; r.argmax_component = comp;
    r.n_free = r_nf[0];
    r.status = bad ? 1 : 0;
    r.pad = 0;
    rec[win] = r;
  }
}

extern "C" int vilo_batch_gradient(vilo_ctx *ctx, vilo_batch *bt, vilo_window_gradient_record *windows, double *state_grad, double *state_diag,
                                   double *lm_grad, double *lm_diag) {
  if (!ctx || !bt || !windows) return VILO_ERR_BAD_ARG;
  if (bt->mask.refuse(ctx, "vilo_batch_gradient") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm;
  BatchCall call(ctx, bt, &vilo_ctx::last_grad_ms);
  // the call's device memory: saved solver state | window records | state gradient | state diagonal | landmark gradient | landmark diagonal
  const size_t o_st = call.lay.take<SolverState>(W), o_rec = call.lay.take<vilo_window_gradient_record>(W);
  const size_t o_sg = call.lay.take<double>(GN_NS * (size_t)W), o_sd = call.lay.take<double>(GN_NS * (size_t)W);
  const size_t o_lg = call.lay.take<double>(n_lm), o_ld = call.lay.take<double>(n_lm);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  const int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  hipLaunchKernelGGL(k_gradient, dim3(W), dim3(GN_T), 0, ctx->stream, bd, call.ptr<vilo_window_gradient_record>(o_rec), call.ptr<double>(o_sg),
                     call.ptr<double>(o_sd), call.ptr<double>(o_lg), call.ptr<double>(o_ld));
  VILO_HIP(hipGetLastError());
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  VILO_HIP(call.down(windows, call.ptr<char>(o_rec), sizeof(vilo_window_gradient_record) * (size_t)W));
  VILO_HIP(call.down(state_grad, call.ptr<char>(o_sg), sizeof(double) * GN_NS * (size_t)W));
  VILO_HIP(call.down(state_diag, call.ptr<char>(o_sd), sizeof(double) * GN_NS * (size_t)W));
  VILO_HIP(call.down(lm_grad, call.ptr<char>(o_lg), sizeof(double) * (size_t)n_lm));
  VILO_HIP(call.down(lm_diag, call.ptr<char>(o_ld), sizeof(double) * (size_t)n_lm));
  return VILO_OK;
}

extern "C" int vilo_window_gradient(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                    vilo_window_gradient_record *windows, double *state_grad, double *state_diag, double *lm_grad, double *lm_diag) {
  if (!ctx || n_windows < 1 || !in || !state || !windows) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state,
                         [&](vilo_batch *bt) { return vilo_batch_gradient(ctx, bt, windows, state_grad, state_diag, lm_grad, lm_diag); });
}

extern "C" double vilo_last_gradient_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_grad_ms : -1.0; }
