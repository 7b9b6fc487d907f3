// Dogleg trust-region step (Ceres' DoglegStrategy, TRADITIONAL_DOGLEG) of every window of a batch at its current device state
// (vilo_batch_dogleg_step, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0), once per call, exactly as vilo_batch_gradient runs it: the
// windows' SolverStates are copied aside before and back after; x, lambda and the prior are only read.
// The Gauss-Newton point: k_gn_step, unchanged, through vilo_gn_step_launch (gn_step_launch.hpp): delta_gn, its record.
//
// k_dogleg, one workgroup per window, one code path for every batch size, all FP64, no floating-point atomics. With M = diag(D^2 / s^2)
// (step_dd), the scaled quantities of the definition are sums in the caller's coordinates: the Cauchy direction c = S u = g / M (under the
// FRAME0 gauge: M's steepest descent inside the gauge's subspace, dg_gauge_cauchy), |g^|^2 = g . c, |p^_gn|^2 = delta_gn^T M delta_gn,
// g^ . p^_gn = g . delta_gn, u^T S H S u = c^T H c, and the step is delta = a c + beta delta_gn. Steps:
//   1. g and h of the 222 state entries by their owners (state_entry_gh of gn_system.hpp); M, c.
//   2. V = [c | delta_gn] into LDS by camera dimension: two columns of k_hess_vec's 16-column tile, the other fourteen zero operands.
//   3. Y = H V exactly as k_hess_vec forms it: P of the visual Gram slots and Y_P = P V_P, the IMU Gram of every interval on its rows,
//      the prior on its rows, then the landmarks 32 per pass (their coupling rows staged once for both columns), Y_P += sum_l w_l v_l on
//      the matrix cores, y_l = E_l v_l + w_l^T v_P by thread (landmark, column).
//   4. the six sums g . c, c^T H c, g . delta_gn, delta_gn^T M delta_gn, delta_gn^T H delta_gn, c^T H delta_gn: thread t takes state entry t
//      and, in step 3, its (landmark, column) of every pass; then one fixed halving tree.
//   5. every thread chooses the branch from the same six numbers; delta = a c + beta delta_gn entry by entry (branch 0: delta_gn's bits);
//      delta^T H delta = a^2 c^T H c + 2 a beta c^T H delta_gn + beta^2 delta_gn^T H delta_gn: no third product.
//   6. |p^|^2 = delta^T M delta and |delta|^2 by a second tree; the record.
// LDS: P 51 200 B (the landmark staging, 21 632 B, and the trees, 12 288 B, reuse its place once P V_P is done) + V 3584 B + Y 3584 B +
// g, M 3584 B + prior dx 768 B + maps 832 B + scalars 128 B = 63 680 B: two workgroups per CU, the smaller of k_hess_vec's two budgets
// (DESIGN 4.35), which __launch_bounds__ asks the registers for.
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "gn_step_launch.hpp"
#include "gn_system.hpp"

static_assert(sizeof(vilo_dogleg_opts) == 32, "vilo_dogleg_opts: 32 bytes (cerberus_amd/_ctypes.py mirrors it)");
static_assert(sizeof(vilo_dogleg_opts) == sizeof(vilo_step_opts) && offsetof(vilo_dogleg_opts, min_pivot) == offsetof(vilo_step_opts, min_pivot),
              "vilo_dogleg_opts: vilo_step_opts' fields");
static_assert(sizeof(vilo_window_dogleg_record) == 80 && offsetof(vilo_window_dogleg_record, branch) == 64 &&
                  offsetof(vilo_window_dogleg_record, status) == 72,
              "vilo_window_dogleg_record: 80 bytes (cerberus_amd/_ctypes.py mirrors it)");

#define DG_K 2              // columns: c, delta_gn
#define DG_LMC 32           // landmarks per pass
#define DG_WS 33            // row stride of the staged coupling rows (k_hess_vec's pad)
#define DG_NSUM 6
// LDS (doubles)
#define DL_P 0                                // [80][80] visual pose block; then: staging | trees
#define DL_WT DL_P                            //   [80][33] w_l of a pass, by camera dimension
#define DL_VL (DL_WT + GN_NP * DG_WS)         //   [32][2] v_l of a pass
#define DL_RED DL_P                           //   [6][256] the trees
#define DL_V (DL_P + GN_NP * GN_NP)           // [224][2] V by camera dimension
#define DL_Y (DL_V + CD_N * DG_K)             // [224][2] Y
#define DL_G (DL_Y + CD_N * DG_K)             // [224] g by camera dimension
#define DL_M (DL_G + CD_N)                    // [224] M by camera dimension
#define DL_DX (DL_M + CD_N)                   // [96] prior dx
#define DL_MAP (DL_DX + VILO_MAX_PRIOR_DIM)   // int pmap[96], short inv_pmap[224]
#define DL_SC (DL_MAP + (96 * 4 + 224 * 2 + 7) / 8)   // [16] Q (9), the sums' flags
#define DL_N (DL_SC + 16)
static_assert(DL_VL + DG_LMC * DG_K <= DL_V && DG_NSUM * GN_T <= GN_NP * GN_NP, "k_dogleg: what reuses P's place");
static_assert(sizeof(double) * DL_N + 64 <= 80 * 1024, "k_dogleg: two workgroups per CU");

// The Cauchy direction of frame 0's rotation under the FRAME0 gauge, by one thread: the minimiser of g . d + d^T M d / 2 over d = E z,
// E = [e1 e2] of gauge_basis: c = E (E^T M E)^-1 E^T g, so that g . c = c^T M c as without a gauge. g, m: the three entries; c out.
__device__ __forceinline__ void dg_gauge_cauchy(const double *Q, const double *g, const double *m, double *c) {
  const double *e1 = Q, *e2 = Q + 3;
  double a11 = 0.0, a12 = 0.0, a22 = 0.0, b1 = 0.0, b2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    a11 += e1[i] * m[i] * e1[i]; a12 += e1[i] * m[i] * e2[i]; a22 += e2[i] * m[i] * e2[i];
    b1 += e1[i] * g[i]; b2 += e2[i] * g[i];
  }
  const double det = a11 * a22 - a12 * a12;
  const double z1 = (a22 * b1 - a12 * b2) / det, z2 = (a11 * b2 - a12 * b1) / det;
  for (int i = 0; i < 3; ++i) c[i] = e1[i] * z1 + e2[i] * z2;
}

// `n` sums of GN_T partial values each, red [n][GN_T]: the halving tree of k_gn_step's record; the sums end in red[i * GN_T]. Barriers inside.
__device__ __forceinline__ void dg_tree(double *red, int n) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int st = GN_T / 2; st > 0; st >>= 1) {
    if (tid < st)
      for (int i = 0; i < n; ++i) red[i * GN_T + tid] += red[i * GN_T + tid + st];
    __syncthreads();
  }
}

__global__ void __launch_bounds__(GN_T, 2) k_dogleg(BatchDev b, int gauge, double lo, double hi, const double *radius_in,
                                                   const vilo_window_step_record *gn_rec, const double *gn_ss, const double *gn_ls,
                                                   vilo_window_dogleg_record *rec, double *ss_out, double *ls_out, double *cs_out, double *cl_out) {
  using namespace vilo;
  extern __shared__ double lds[];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const WinMeta wm = b.win[w];
  const int F = wm.n_frames, L = wm.L;
  double *Pm = lds + DL_P, *Wt = lds + DL_WT, *Vl = lds + DL_VL, *red = lds + DL_RED, *Vs = lds + DL_V, *Ys = lds + DL_Y, *gs = lds + DL_G, *ms = lds + DL_M,
         *dxs = lds + DL_DX, *Q = lds + DL_SC;
  int *pmap = (int *)(lds + DL_MAP);
  short *inv_pmap = (short *)(pmap + 96);
  double *so = ss_out + (size_t)w * GN_NS, *lo_out = ls_out + wm.lm_off;
  double *co = cs_out ? cs_out + (size_t)w * GN_NS : nullptr, *cl = cl_out ? cl_out + wm.lm_off : nullptr;
  const double *dgs = gn_ss + (size_t)w * GN_NS, *dgl = gn_ls + wm.lm_off;
  const vilo_window_step_record gr = gn_rec[w];
  const double radius = radius_in[w];
  // every output of the window NaN, the record's counts kept (uniform: decided from what every thread read alike)
  auto fail = [&](int status) {
    for (int e = tid; e < GN_NS; e += GN_T) { so[e] = NAN; if (co) co[e] = NAN; }
    for (int l = tid; l < L; l += GN_T) { lo_out[l] = NAN; if (cl) cl[l] = NAN; }
    if (tid == 0) {
      vilo_window_dogleg_record r;
      r.alpha = NAN; r.gradient_norm = NAN; r.gauss_newton_norm = NAN; r.step_norm = NAN; r.beta = NAN; r.model_cost_change = NAN;
      r.grad_dot_step = NAN; r.norm = NAN;
      r.branch = -1; r.n_free = gr.n_free; r.status = status; r.pad = 0;
      rec[w] = r;
    }
  };
  if (gr.status != 0) { fail(gr.status); return; }   // (invalid window, bad mu, a failed solve: k_gn_step's status)
  if (!(radius > 0.0) || !isfinite(radius)) { fail(1); return; }
  const bool frame0 = gauge == VILO_COV_GAUGE_FRAME0;
  const int pn = wm.prior_n;
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Pm[e] = 0.0;
  for (int e = tid; e < CD_N * DG_K; e += GN_T) { Vs[e] = 0.0; Ys[e] = 0.0; }
  for (int e = tid; e < CD_N; e += GN_T) { gs[e] = 0.0; ms[e] = 0.0; }
  if (tid < 96) pmap[tid] = tid < pn ? b.prior_map[(size_t)w * 96 + tid] : 0;
  prior_view_init(b, wm, w, pmap, dxs, inv_pmap);

  // ---- 1. g, h, M of the 222 state entries ----
  double g = 0.0, m = 0.0, c = 0.0, d = 0.0;
  bool act = false;
  const int cd = tid < GN_NS ? caller_cd(tid) : CD_N - 1;
  if (tid < GN_NS) {
    act = cd_active(cd, F, wm.const_mask);
    if (act) {
      double h = 0.0;
      state_entry_gh<true>(b, wm, w, cd, inv_pmap, dxs, g, h);
      m = step_dd(h, lo, hi);
      c = g / m;
      d = dgs[tid];
      gs[cd] = g;
      ms[cd] = m;
    }
  }
  if (frame0 && tid == 0) gauge_basis(b.x + (size_t)w * XSTRIDE + XO_POSE + 3, Q);
  __syncthreads();
  // ---- 2. V = [c | delta_gn] ----
  if (frame0 && act && cd < 6) {   // frame 0's position is held; its rotation moves in [e1 e2]
    if (cd < 3) c = 0.0;
    else {
      double c3[3];
      dg_gauge_cauchy(Q, gs + 3, ms + 3, c3);
      c = c3[cd - 3];
    }
  }
  if (act) { Vs[cd * DG_K] = c; Vs[cd * DG_K + 1] = d; }

  // ---- 3. Y = H V ----
  assemble_visual_pose_block(b, wm, Pm);
  __syncthreads();
  auto vcol = [&](int kk, int col) { return col < DG_K ? Vs[kk * DG_K + col] : 0.0; };
  for (int X = wave; X < 5; X += 4) {   // (wave-uniform; P is symmetric: read down a column, lane by lane)
    const mfma_d4 acc = hv_tile(16 * X, GN_NP / 4, lr, lk, [&](int i, int kk) { return Pm[kk * GN_NP + i]; }, vcol);
    if (lr < DG_K) {
#pragma unroll
      for (int r = 0; r < 4; ++r) Ys[(16 * X + lk + 4 * r) * DG_K + lr] = acc[r];
    }
  }
  __syncthreads();
  for (int k = 0; k + 1 < F && k < VILO_WINDOW_SIZE; ++k) {
    if (b.imu_skip[w * 10 + k]) continue;   // (uniform)
    if (wave < 3) {
      const double *gm = b.imu_gram + (size_t)(w * 10 + k) * 780;
      const mfma_d4 acc = hv_tile(16 * wave, 10, lr, lk,
                                  [&](int i, int kk) { return (i < 38 && kk < 38) ? gm[tri39(min(i, kk), max(i, kk))] : 0.0; },
                                  [&](int kk, int col) { return kk < 38 ? vcol(hv_imu_cd(k, kk), col) : 0.0; });
      if (lr < DG_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * wave + lk + 4 * r;
          if (row < 38) Ys[hv_imu_cd(k, row) * DG_K + lr] += acc[r];
        }
      }
    }
    __syncthreads();
  }
  if (pn > 0) {
    const double *Hp = b.prior_H + (size_t)w * 96 * 96;
    for (int X = wave; 16 * X < pn; X += 4) {
      const mfma_d4 acc = hv_tile(16 * X, (pn + 3) / 4, lr, lk, [&](int i, int kk) { return (i < pn && kk < pn) ? Hp[(size_t)kk * pn + i] : 0.0; },
                                  [&](int kk, int col) { return kk < pn ? vcol(pmap[kk], col) : 0.0; });
      if (lr < DG_K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * X + lk + 4 * r;
          if (row < pn) Ys[pmap[row] * DG_K + lr] += acc[r];
        }
      }
    }
  }
  __syncthreads();   // (P is done with: its place is the landmark staging below)

  // the landmarks; thread (li, col) of the first 64 takes landmark l0 + li of every pass in column col
  double a_s[DG_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // g.c, cHc, g.d, dMd, dHd, cHd
  const double *wl = b.lm_w + 80 * (size_t)wm.lm_off, *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
  const int *perm = b.lm_perm + wm.lm_off;
  {
    const int li = tid & 31, col = tid >> 5;
    mfma_d4 accP[2] = {mfma_d4{0.0, 0.0, 0.0, 0.0}, mfma_d4{0.0, 0.0, 0.0, 0.0}};   // tile `wave` of Y_P; wave 0: tile 4 too
    for (int l0 = 0; l0 < L; l0 += DG_LMC) {
      const int nl = min(DG_LMC, L - l0);
      for (int e = tid; e < GN_NP * DG_LMC; e += GN_T) {
        const int l = e % DG_LMC, a = e / DG_LMC;
        Wt[a * DG_WS + l] = (l < nl && a < VILO_NPU) ? wl[(size_t)a * L + l0 + l] : 0.0;
      }
      if (tid < DG_LMC) {
        double vc = 0.0, vd = 0.0;
        if (tid < nl) {
          vc = lmg[l0 + tid] / step_dd(lmE[l0 + tid], lo, hi);
          vd = dgl[perm[l0 + tid]];
        }
        Vl[tid * DG_K] = vc;
        Vl[tid * DG_K + 1] = vd;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int X = wave + 4 * i;
        if (X < 5) {   // (wave-uniform)
          for (int ks = 0; ks < DG_LMC / 4; ++ks) {
            const int kk = 4 * ks + lk;
            accP[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[(16 * X + lr) * DG_WS + kk], lr < DG_K ? Vl[kk * DG_K + lr] : 0.0, accP[i], 0, 0, 0);
          }
        }
      }
      if (col < DG_K && li < nl) {
        const int l = l0 + li;
        const double E = lmE[l], gl = lmg[l], ml = step_dd(E, lo, hi);
        const double vc = Vl[li * DG_K], vd = Vl[li * DG_K + 1], v = col == 0 ? vc : vd;
        double y = E * v;
        for (int a = 0; a < VILO_NPU; ++a) y = fma(Wt[a * DG_WS + li], Vs[a * DG_K + col], y);
        if (col == 0) {
          a_s[0] = fma(gl, vc, a_s[0]);
          a_s[1] = fma(vc, y, a_s[1]);
        } else {
          a_s[2] = fma(gl, vd, a_s[2]);
          a_s[3] = fma(ml * vd, vd, a_s[3]);
          a_s[4] = fma(vd, y, a_s[4]);
          a_s[5] = fma(vc, y, a_s[5]);
        }
      }
      __syncthreads();
    }
    if (lr < DG_K) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int X = wave + 4 * i;
        if (X < 5) {
#pragma unroll
          for (int r = 0; r < 4; ++r) Ys[(16 * X + lk + 4 * r) * DG_K + lr] += accP[i][r];
        }
      }
    }
  }
  __syncthreads();

  // ---- 4. the six sums ----
  if (act) {
    const double yc = Ys[cd * DG_K], yd = Ys[cd * DG_K + 1];
    a_s[0] = fma(g, c, a_s[0]);
    a_s[1] = fma(c, yc, a_s[1]);
    a_s[2] = fma(g, d, a_s[2]);
    a_s[3] = fma(m * d, d, a_s[3]);
    a_s[4] = fma(d, yd, a_s[4]);
    a_s[5] = fma(c, yd, a_s[5]);
  }
#pragma unroll
  for (int i = 0; i < DG_NSUM; ++i) red[i * GN_T + tid] = a_s[i];
  dg_tree(red, DG_NSUM);
  const double gg = red[0], cHc = red[GN_T], gd = red[2 * GN_T], pp = red[3 * GN_T], dHd = red[4 * GN_T], cHd = red[5 * GN_T];
  __syncthreads();   // (the second tree writes the same place)

  // ---- 5. the branch and the step (every thread, from the same numbers) ----
  const double alpha = gg / cHc, gnorm = sqrt(gg), gn_norm = gr.scaled_norm;
  int branch;
  double a, beta;   // p^ = a g^ + beta p^_gn
  if (gn_norm <= radius) { branch = 0; a = 0.0; beta = 1.0; }
  else if (gnorm * alpha >= radius) { branch = 1; a = -(radius / gnorm); beta = 0.0; }
  else {
    branch = 2;
    const double b_dot_a = -alpha * gd, a_sq = (alpha * gnorm) * (alpha * gnorm);
    const double bma = a_sq - 2.0 * b_dot_a + pp;
    const double cc = b_dot_a - a_sq;
    const double dd = sqrt(cc * cc + bma * (radius * radius - a_sq));
    beta = (cc <= 0.0) ? (dd - cc) / bma : (radius * radius - a_sq) / (dd + cc);
    a = -alpha * (1.0 - beta);
  }
  double s_sq = 0.0, s_mm = 0.0, s_bad = 0.0;
  double ds = 0.0, dc = 0.0;
  if (act) {
    ds = branch == 0 ? d : a * c + beta * d;
    dc = -alpha * c;
    s_sq = ds * ds; s_mm = m * ds * ds;
    if (!isfinite(ds) || !isfinite(dc)) s_bad = 1.0;
  }
  for (int l = tid; l < L; l += GN_T) {
    const double ml = step_dd(lmE[l], lo, hi), cl_ = lmg[l] / ml, dl = dgl[perm[l]];
    const double s = branch == 0 ? dl : a * cl_ + beta * dl, sc = -alpha * cl_;
    lo_out[perm[l]] = s;
    if (cl) cl[perm[l]] = sc;
    s_sq = fma(s, s, s_sq); s_mm = fma(ml * s, s, s_mm);
    if (!isfinite(s) || !isfinite(sc)) s_bad = 1.0;
  }

  // ---- 6. the norms and the record ----
  red[tid] = s_sq; red[GN_T + tid] = s_mm; red[2 * GN_T + tid] = s_bad;
  dg_tree(red, 3);
  const double gdot = a * gg + beta * gd;
  const double sHs = a * a * cHc + 2.0 * a * beta * cHd + beta * beta * dHd;
  const double mcc = -(gdot + 0.5 * sHs);
  const double pnorm = branch == 0 ? gn_norm : (branch == 1 ? radius : sqrt(red[GN_T]));
  const bool bad = red[2 * GN_T] != 0.0 || !isfinite(alpha) || !isfinite(gnorm) || !isfinite(gn_norm) || !isfinite(beta) || !isfinite(mcc) || !isfinite(pnorm);
  if (bad) { fail(1); return; }   // (uniform; fail writes every entry, the landmarks' too)
  if (tid < GN_NS) { so[tid] = ds; if (co) co[tid] = dc; }
  if (tid == 0) {
    vilo_window_dogleg_record r;
    r.alpha = alpha; r.gradient_norm = gnorm; r.gauss_newton_norm = gn_norm; r.step_norm = pnorm; r.beta = beta; r.model_cost_change = mcc;
    r.grad_dot_step = gdot; r.norm = sqrt(red[0]);
    r.branch = branch; r.n_free = gr.n_free; r.status = 0; r.pad = 0;
    rec[w] = r;
  }
}

extern "C" void vilo_default_dogleg_opts(vilo_dogleg_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->gauge = VILO_COV_GAUGE_NONE;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_pivot = 1e-14;
}

extern "C" double vilo_last_dogleg_step_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_dogleg_step_ms : -1.0; }

extern "C" int vilo_batch_dogleg_step(vilo_ctx *ctx, vilo_batch *bt, const vilo_dogleg_opts *opts, const double *radius, const double *mu,
                                      vilo_window_dogleg_record *windows, double *state_step, double *lm_step, double *cauchy_state, double *cauchy_lm) {
  if (!ctx || !bt || !windows || !radius) return VILO_ERR_BAD_ARG;
  if (bt->mask.refuse(ctx, "vilo_batch_dogleg_step") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  vilo_dogleg_opts od;
  if (opts) od = *opts; else vilo_default_dogleg_opts(&od);
  vilo_step_opts o;
  o.gauge = od.gauge; o.pad0 = od.pad0; o.min_lm_diagonal = od.min_lm_diagonal; o.max_lm_diagonal = od.max_lm_diagonal; o.min_pivot = od.min_pivot;
  if (!vilo_step_opts_ok(o)) {
    ctx->err = "vilo_batch_dogleg_step: bad options (gauge, pad0 == 0, 0 <= min_lm_diagonal <= max_lm_diagonal < inf, min_pivot >= 0)";
    return VILO_ERR_BAD_ARG;
  }
  BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm;
  const bool want_c = cauchy_state != nullptr || cauchy_lm != nullptr;
  BatchCall call(ctx, bt, &vilo_ctx::last_dogleg_step_ms);
  // the call's device memory: saved solver state | k_gn_step's blocks | radius | records | state step | landmark step | the Cauchy points
  const size_t o_st = call.lay.take<SolverState>(W);
  const GnStepBlocks gb(call.lay, bd, mu != nullptr);
  const size_t o_rad = call.lay.take<double>(W), o_rec = call.lay.take<vilo_window_dogleg_record>(W);
  const size_t o_ss = call.lay.take<double>(GN_NS * (size_t)W), o_ls = call.lay.take<double>(n_lm);
  const size_t o_cs = call.lay.take<double>(GN_NS * (size_t)W, want_c), o_cl = call.lay.take<double>(n_lm, want_c);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  if (!ctx->dogleg_attr_set) {
    VILO_HIP(hipFuncSetAttribute((const void *)k_dogleg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * DL_N)));
    ctx->dogleg_attr_set = true;
  }
  if (mu) VILO_HIP(hipMemcpy(call.ptr<double>(gb.o_mu), mu, sizeof(double) * (size_t)W, hipMemcpyHostToDevice));
  VILO_HIP(hipMemcpy(call.ptr<double>(o_rad), radius, sizeof(double) * (size_t)W, hipMemcpyHostToDevice));
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  rc = vilo_gn_step_launch(ctx, call, bd, gb, o);
  if (rc != VILO_OK) return rc;
  // k_dogleg alone, for vilo_get_kernel_times (vilo_set_profiling)
  const bool timed = ctx->profile == 1 || ctx->profile == 2 + VILO_K_DOGLEG;
  hipEvent_t pe[2] = {nullptr, nullptr};
  if (timed) {
    VILO_HIP(hipEventCreate(&pe[0]));
    VILO_HIP(hipEventCreate(&pe[1]));
    VILO_HIP(hipEventRecord(pe[0], ctx->stream));
  }
  hipLaunchKernelGGL(k_dogleg, dim3(W), dim3(GN_T), sizeof(double) * DL_N, ctx->stream, bd, o.gauge, o.min_lm_diagonal, o.max_lm_diagonal,
                     call.ptr<double>(o_rad), call.ptr<vilo_window_step_record>(gb.o_rec),
                     call.ptr<double>(gb.o_ss), call.ptr<double>(gb.o_ls), call.ptr<vilo_window_dogleg_record>(o_rec), call.ptr<double>(o_ss),
                     call.ptr<double>(o_ls), want_c ? call.ptr<double>(o_cs) : (double *)nullptr, want_c ? call.ptr<double>(o_cl) : (double *)nullptr);
  VILO_HIP(hipGetLastError());
  if (timed) VILO_HIP(hipEventRecord(pe[1], ctx->stream));
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  if (timed) {
    float t = 0.f;
    VILO_HIP(hipEventElapsedTime(&t, pe[0], pe[1]));
    ctx->kernel_ms[VILO_K_DOGLEG] += t;
    ctx->kernel_launches[VILO_K_DOGLEG] += 1;
    (void)hipEventDestroy(pe[0]);
    (void)hipEventDestroy(pe[1]);
  }
  VILO_HIP(call.down(windows, call.ptr<char>(o_rec), sizeof(vilo_window_dogleg_record) * (size_t)W));
  VILO_HIP(call.down(state_step, call.ptr<char>(o_ss), sizeof(double) * GN_NS * (size_t)W));
  VILO_HIP(call.down(lm_step, call.ptr<char>(o_ls), sizeof(double) * (size_t)n_lm));
  VILO_HIP(call.down(cauchy_state, call.ptr<char>(o_cs), sizeof(double) * GN_NS * (size_t)W));
  VILO_HIP(call.down(cauchy_lm, call.ptr<char>(o_cl), sizeof(double) * (size_t)n_lm));
  return VILO_OK;
}

extern "C" int vilo_window_dogleg_step(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_dogleg_opts *opts,
                                       const double *radius, const double *mu, vilo_window_dogleg_record *windows, double *state_step, double *lm_step,
                                       double *cauchy_state, double *cauchy_lm) {
  if (!ctx || n_windows < 1 || !in || !state || !windows || !radius) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_dogleg_step(ctx, bt, opts, radius, mu, windows, state_step, lm_step, cauchy_state, cauchy_lm);
  });
}
