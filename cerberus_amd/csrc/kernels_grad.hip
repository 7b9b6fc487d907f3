// Cost gradient and Gauss-Newton diagonal of every window of a batch at its current device state (vilo_batch_gradient, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0), exactly as vilo_batch_covariance runs it: the windows'
// SolverStates are copied aside before and back after; x, lambda and the prior are only read. No factor is evaluated here: J^T r and
// diag(J^T J) are in what that pass leaves — the r column and the diagonal of the 23-column visual Gram slots and of the 39 x 39 IMU
// Grams, lm_gbuf[0] / lm_E for the inverse depths — and in the prior's H, b0 and H dx.
//
// k_gradient, one workgroup per window, one code path for every batch size, all FP64:
//   1. owner-computes: thread d < 222 owns output dimension d of the caller's layout (pose 11 x 6, speed-bias 11 x 9, leg bias 11 x 4,
//      extrinsics 2 x 6, td) and walks its contributions in one fixed order — the window's visual Gram slots (chunks ascending, frame
//      offsets ascending, through gram26_index), the IMU Gram of interval k - 1 then of interval k, the prior's b0 + H dx and diag H —
//      with plain adds in a register. No floating-point atomics; nothing depends on the batch a window shares or on its position.
//   2. the landmarks' lm_g / lm_E go to the caller's order (lm_off + lm_perm).
//   3. the window record: thread t takes entries t, t + 256, ... of the list [222 state entries | the landmarks in caller order], then one
//      fixed halving tree over the threads (sum of squares, max |g| with its position — ties to the lower position —, max |g| / sqrt(h),
//      the count of free coordinates, a not-finite flag).
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "solve_common.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_window_gradient_record) == 48, "vilo_window_gradient_record: 48 bytes (include/vilo_gpu.h)");

#define GR_T 256
#define GR_NS 222   // state entries per window (VILO_NCAM)

// camera dimension (solver_types.hpp) of entry d of the caller's layout
__device__ __forceinline__ int grad_cd(int d) {
  if (d < 66) return d;
  if (d < 165) { const int k = (d - 66) / 9; return CD_B0 + 13 * k + (d - 66 - 9 * k); }
  if (d < 209) { const int k = (d - 165) / 4; return CD_B0 + 13 * k + 9 + (d - 165 - 4 * k); }
  if (d < 221) return CD_EX0 + (d - 209);
  return CD_TD;
}

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

__global__ void __launch_bounds__(GR_T) k_gradient(BatchDev b, vilo_window_gradient_record *rec, double *sg_out, double *sd_out, double *lg_out,
                                                  double *ld_out) {
  using namespace vilo;
  __shared__ double dxs[VILO_MAX_PRIOR_DIM];
  __shared__ short inv_pmap[CD_N];
  __shared__ double r_sq[GR_T], r_mx[GR_T], r_sc[GR_T];
  __shared__ int r_pos[GR_T], r_nf[GR_T], r_bad[GR_T];
  const int win = blockIdx.x, tid = threadIdx.x;
  const WinMeta wm = b.win[win];
  const int F = wm.n_frames, L = wm.L;
  double *sg = sg_out + (size_t)win * GR_NS, *sd = sd_out + (size_t)win * GR_NS;
  double *lg = lg_out + wm.lm_off, *ld = ld_out + wm.lm_off;
  if (b.win_bad && b.win_bad[win]) {   // a preintegration covariance without sqrt_info: the window is not linearised (k_init_state marks it done)
    for (int e = tid; e < GR_NS; e += GR_T) { sg[e] = NAN; sd[e] = NAN; }
    for (int l = tid; l < L; l += GR_T) { lg[l] = NAN; ld[l] = NAN; }
    if (tid == 0) {
      vilo_window_gradient_record r;
      r.max_norm = NAN; r.norm = NAN; r.scaled_max = NAN;
      r.argmax_kind = -1; r.argmax_index = -1; r.argmax_component = -1;
      r.n_free = 0; r.status = 2; r.pad = 0;
      rec[win] = r;
    }
    return;
  }
  const int pn = wm.prior_n;
  for (int e = tid; e < CD_N; e += GR_T) inv_pmap[e] = -1;
  if (pn > 0 && tid < wm.prior_nb)
    prior_dx(b.x + (size_t)win * XSTRIDE + b.prior_bstate[win * 40 + tid], b.prior_x0 + (size_t)win * 280 + b.prior_bxoff[win * 40 + tid],
             b.prior_bsize[win * 40 + tid], dxs + b.prior_bidx[win * 40 + tid]);
  __syncthreads();
  if (tid < pn) inv_pmap[b.prior_map[(size_t)win * 96 + tid]] = (short)tid;
  __syncthreads();

  // ---- 1. the 222 state entries ----
  double g = 0.0, h = 0.0;
  bool act = false;
  if (tid < GR_NS) {
    const int cd = grad_cd(tid);
    act = cd_active(cd, F, wm.const_mask);
    if (act) {
      if (cd < CD_B0) {
        // visual Gram slots, the 26-column view [pose_s 6 | pose_j 6 | ex0 6 | ex1 6 | td | r]: a pose dimension of frame f is column a of the
        // chunks that start in f (every frame offset) and column 6 + a of offset f - s of the chunks that start before it
        const int f = cd / 6, a = cd - 6 * f;
        const int crest = cd < 66 ? -1 : (cd < CD_TD ? 12 + (cd - CD_EX0) : 24);
        for (int ch = 0; ch < wm.n_chunks; ++ch) {
          const ChunkMeta cm = b.chunk[wm.chunk_off + ch];
          int t0 = 0, t1 = cm.kmax, c = crest;
          if (cd < 66) {
            if (f == cm.s) c = a;
            else if (f > cm.s && f - cm.s < cm.kmax) { c = 6 + a; t0 = f - cm.s; t1 = t0 + 1; }
            else continue;
          }
          double sgn, one;
          const int eg = gram26_index(c, 25, sgn), eh = gram26_index(c, c, one);
          for (int t = t0; t < t1; ++t) {
            const double *gs = b.gram + (size_t)(cm.gram_off + t) * VILO_GRAM;
            g += sgn * gs[eg];
            h += gs[eh];
          }
        }
      }
      // IMU(-leg) Grams [pose_i 6 | B_i 13 | pose_j 6 | B_j 13 | r]: frame f is the "j" of interval f - 1 and the "i" of interval f
      {
        int f, ci;
        if (cd < 66) { f = cd / 6; ci = cd - 6 * f; }
        else if (cd >= CD_B0) { f = (cd - CD_B0) / 13; ci = 6 + (cd - CD_B0 - 13 * f); }
        else { f = -1; ci = 0; }
        if (f >= 0) {
          if (f >= 1 && !b.imu_skip[win * 10 + f - 1]) {
            const double *gr = b.imu_gram + (size_t)(win * 10 + f - 1) * 780;
            g += gr[tri39(19 + ci, 38)];
            h += gr[tri39(19 + ci, 19 + ci)];
          }
          if (f + 1 < F && f < VILO_WINDOW_SIZE && !b.imu_skip[win * 10 + f]) {
            const double *gr = b.imu_gram + (size_t)(win * 10 + f) * 780;
            g += gr[tri39(ci, 38)];
            h += gr[tri39(ci, ci)];
          }
        }
      }
      // prior: J^T r = b0 + H dx, diag(J^T J) = diag H
      const int pi = inv_pmap[cd];
      if (pn > 0 && pi >= 0) {
        const double *Hp = b.prior_H + (size_t)win * 96 * 96;
        double s = b.prior_b0[(size_t)win * 96 + pi];
        for (int q = 0; q < pn; ++q) s += Hp[(size_t)q * pn + pi] * dxs[q];
        g += s;
        h += Hp[(size_t)pi * pn + pi];
      }
    }
    sg[tid] = g;
    sd[tid] = h;
  }
  // ---- 2. landmarks to the caller's order ----
  {
    const double *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
    const int *perm = b.lm_perm + wm.lm_off;
    for (int l = tid; l < L; l += GR_T) {
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
  for (int e = tid; e < L; e += GR_T) grad_take(p, GR_NS + e, lg[e], ld[e]);   // (positions tid + 256 m ascend with m: GR_NS + e > tid)
  r_sq[tid] = p.sq; r_mx[tid] = p.mx; r_sc[tid] = p.sc; r_pos[tid] = p.pos; r_nf[tid] = p.nfree; r_bad[tid] = p.bad;
  __syncthreads();
  for (int st = GR_T / 2; st > 0; st >>= 1) {
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
      else { kind = VILO_BLK_FEAT; idx = pos - GR_NS; comp = 0; }
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
  const size_t o_sg = call.lay.take<double>(GR_NS * (size_t)W), o_sd = call.lay.take<double>(GR_NS * (size_t)W);
  const size_t o_lg = call.lay.take<double>(n_lm), o_ld = call.lay.take<double>(n_lm);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  const int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  hipLaunchKernelGGL(k_gradient, dim3(W), dim3(GR_T), 0, ctx->stream, bd, call.ptr<vilo_window_gradient_record>(o_rec), call.ptr<double>(o_sg),
                     call.ptr<double>(o_sd), call.ptr<double>(o_lg), call.ptr<double>(o_ld));
  VILO_HIP(hipGetLastError());
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  VILO_HIP(call.down(windows, call.ptr<char>(o_rec), sizeof(vilo_window_gradient_record) * (size_t)W));
  VILO_HIP(call.down(state_grad, call.ptr<char>(o_sg), sizeof(double) * GR_NS * (size_t)W));
  VILO_HIP(call.down(state_diag, call.ptr<char>(o_sd), sizeof(double) * GR_NS * (size_t)W));
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
