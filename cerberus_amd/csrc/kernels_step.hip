// Gauss-Newton / damped step of every window of a batch at its current device state (vilo_batch_gauss_newton_step, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0), exactly as vilo_batch_gradient and vilo_batch_covariance run it:
// the windows' SolverStates are copied aside before and back after; x, lambda and the prior are only read.
//
// k_gn_step, one workgroup per window, one code path for every batch size, all FP64. The camera-side dimensions split as gn_system.hpp
// splits them: P (79 + 1 padding, LDS), B (11 x 13, block tridiagonal), BP (143 x 80, global scratch or LDS: the forms below). The reading
// of the linearisation (owner walk, assembly, gauge, scaling, 13 x 13 Cholesky) is gn_system.hpp's. Steps:
//   1. owner-computes g and h = diag(H) of the 222 state entries (state_entry_gh); dd_i = D^2_i / s_i^2 from h_i.
//   2. assembly of H (assemble_visual_pose_block, assemble_imu_grams, assemble_prior), mu dd on the diagonal; the landmarks are
//      eliminated with the damped E~_l = E_l + mu dd_l: P -= W^T W on the FP64 matrix cores (W = w_l^T / sqrt(E~_l), 32 or 16 landmarks per
//      pass staged in LDS), g_P -= sum w_l g_l / E~_l.
//   3. FRAME0 gauge: frame 0's rotation rows / columns and right-hand side in the basis [e1 e2 u] (gauge_basis); u and frame 0's position
//      become constant dimensions.
//   4. Jacobi equilibration (unit diagonal of the damped, reduced camera system); a constant or absent dimension gets scale 0, a unit
//      pivot and a zero right-hand side.
//   5. forward over the chain: L_k (Cholesky of B_kk - T_k T_k^T), T_k = A_{k,k-1} L_{k-1}^-T and Y_k = L_k^-1 (BP_k - T_k Y_{k-1}) by
//      triangular substitution (column p of Y_k by thread p, in registers), S_P = P - sum Y_k^T Y_k on the matrix cores (16 x 16 x 4
//      tiles, 4 k-steps per frame: rows 13 .. 15 zero), the right-hand side carried along. Cholesky of S_P with the forward substitution of its right-hand side fused into the column
//      loop, one backward substitution, u = y_B - Y x_P, backward over the chain with L_k^T and T_{k+1}^T.
//   6. the step is scaled back (and turned back from [e1 e2 u]); the landmarks' delta_l = -(g_l + w_l^T delta_P) / E~_l, lane = landmark;
//      outputs in the caller's order (state_grad's layout, lm_off + lm_perm).
//   7. the record: thread t takes state entry t and landmarks t, t + 256, ... (device order), then one fixed halving tree.
// No inverse is formed: no L^-1, no Sigma_PP. Two forms of one kernel (template parameter, vilo_set_gn_step_form), the same arithmetic but
// for the split of the landmark passes:
//   streamed (default)  BP / Y in per-call global scratch. LDS: P 51 200 B + one 20 480 B region (prior dx / 32 landmarks of staging / the
//                       chain's Y_k / the record's tree) + three 13 x 13 blocks (4056 B) + two vectors of 224 (3584 B) + Q (128 B) = 79 448 B
//                       (+ 4 B static): two workgroups per CU.
//   resident            BP / Y in LDS (91 520 B), the shared region 10 240 B (16 landmarks of staging): 160 728 B, one workgroup per CU.
// Scratch in global memory per window (the chain's blocks, BP / Y) is per-call memory of the batch's arena; windows go through it in chunks,
// as in k_covariance. DESIGN 4.27 has both forms' times.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "batch_call.hpp"
#include "gn_step_launch.hpp"
#include "gn_system.hpp"

static_assert(sizeof(vilo_step_opts) == 32, "vilo_step_opts: 32 bytes (cerberus_amd/_ctypes.py mirrors it)");
static_assert(sizeof(vilo_window_step_record) == 40, "vilo_window_step_record: 40 bytes (cerberus_amd/_ctypes.py mirrors it)");

#define ST_CHUNK 4096       // windows per scratch pass
// global scratch per window (doubles)
#define SS_BD 0                              // [11][13][13] diagonal blocks of B
#define SS_AO (SS_BD + 11 * 169)             // [11][13][13] A_{k,k-1}, k >= 1
#define SS_L (SS_AO + 11 * 169)              // [11][13][13] L_k (lower triangle)
#define SS_T (SS_L + 11 * 169)               // [11][13][13] T_k = A_{k,k-1} L_{k-1}^-T
#define SS_BP (SS_T + 11 * 169)              // [143][80] BP, then Y
#define SS_N (SS_BP + 143 * GN_NP)
// LDS (doubles)
#define SL_P 0                               // [80][80] pose system, then its Cholesky factor
#define SL_SM (SL_P + GN_NP * GN_NP)         // three 13 x 13: lc, lp, tn (lc also: 1 / sqrt(E~) and g_l / sqrt(E~) of a staging pass)
#define SL_D (SL_SM + 3 * 169)               // [224] scale of every camera dimension (0: constant / absent)
#define SL_B (SL_D + CD_N)                   // [224] g, then the scaled right-hand side, then the solution, by camera dimension
#define SL_Q (SL_B + CD_N)                   // [16] Q = [e1 e2 u] (column-major, 9 used)
#define SL_R (SL_Q + 16)                     // [LMC][80]: prior dx + inverse prior map | landmark staging | Mg [16][80] | the tree
// landmarks per staging pass, LDS doubles and the place of BP of a form (resident: BP / Y behind the shared region)
template <bool YL> struct StepForm {
  static constexpr int LMC = YL ? 16 : 32;
  static constexpr int Y = SL_R + LMC * GN_NP;
  static constexpr int N = Y + (YL ? 143 * GN_NP : 0);
};
static_assert(sizeof(double) * StepForm<false>::N + 64 <= 80 * 1024, "k_gn_step, streamed: two workgroups per CU");
static_assert(sizeof(double) * StepForm<true>::N + 64 <= 160 * 1024, "k_gn_step, resident: the CU's LDS");
static_assert(16 * GN_NP <= StepForm<true>::LMC * GN_NP && 4 * GN_T <= StepForm<true>::LMC * GN_NP && VILO_MAX_PRIOR_DIM + CD_N / 4 <= 16 * GN_NP,
              "k_gn_step: the shared region");

// P -= A^T A for A [4 nk][80] row-major in LDS: the 25 16 x 16 tiles (X = t / 5, Y = t % 5) over the four waves, tile t to wave t % 4.
// Operands of v_mfma_f64_16x16x4f64: lane (lr, lk) gives A^T[16 X + lr][4 ks + lk] and A[4 ks + lk][16 Y + lr]; accumulator r is row
// 16 X + lk + 4 r, column 16 Y + lr (as k_landmark_covariance).
template <int WV>
__device__ __forceinline__ void step_syrk_wave(double *Pm, const double *A, int nk, int lr, int lk) {
  constexpr int NT = (25 - WV + 3) / 4;
  mfma_d4 acc[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) acc[i] = mfma_d4{0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < nk; ++ks) {
    const double *row = A + (4 * ks + lk) * GN_NP + lr;
    double v[5];
#pragma unroll
    for (int X = 0; X < 5; ++X) v[X] = row[16 * X];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const int t = WV + 4 * i;
      acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(v[t / 5], v[t % 5], acc[i], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const int t = WV + 4 * i, X = t / 5, Y = t % 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) Pm[(16 * X + lk + 4 * r) * GN_NP + 16 * Y + lr] -= acc[i][r];
  }
}
__device__ __forceinline__ void step_syrk(double *Pm, const double *A, int nk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lr = lane & 15, lk = lane >> 4;
  switch (wave) {   // (wave-uniform)
    case 0: step_syrk_wave<0>(Pm, A, nk, lr, lk); break;
    case 1: step_syrk_wave<1>(Pm, A, nk, lr, lk); break;
    case 2: step_syrk_wave<2>(Pm, A, nk, lr, lk); break;
    default: step_syrk_wave<3>(Pm, A, nk, lr, lk); break;
  }
}

template <bool YL>
__global__ void __launch_bounds__(GN_T) k_gn_step(BatchDev b, int w0, int gauge, double lo, double hi, double thr, const double *mu_in, double *scr,
                                                 vilo_window_step_record *rec, double *ss_out, double *ls_out) {
  using namespace vilo;
  extern __shared__ double lds[];
  __shared__ int bad_s;
  const int w = w0 + blockIdx.x, tid = threadIdx.x;
  const WinMeta wm = b.win[w];
  const int F = wm.n_frames, L = wm.L;
  constexpr int ST_LMC = StepForm<YL>::LMC;
  double *Pm = lds + SL_P, *Rg = lds + SL_R, *Mg = Rg, *dsc = lds + SL_D, *bv = lds + SL_B, *Q = lds + SL_Q;
  double *lc = lds + SL_SM, *lp = lc + 169, *tn = lp + 169;
  double *G = scr + (size_t)blockIdx.x * SS_N;
  double *Bd = G + SS_BD, *Ao = G + SS_AO, *Lg = G + SS_L, *Tg = G + SS_T, *BP = YL ? lds + StepForm<YL>::Y : G + SS_BP;
  double *so = ss_out + (size_t)w * GN_NS, *lo_out = ls_out + wm.lm_off;
  const double mu = mu_in ? mu_in[w] : 0.0;
  const bool invalid = b.win_bad && b.win_bad[w];
  if (invalid || !(mu >= 0.0) || !isfinite(mu)) {   // a record without sqrt_info (the window is not linearised), or a bad mu: NaN for this window
    for (int e = tid; e < GN_NS; e += GN_T) so[e] = NAN;
    for (int l = tid; l < L; l += GN_T) lo_out[l] = NAN;
    if (tid == 0) {
      vilo_window_step_record r;
      r.model_cost_change = NAN; r.scaled_norm = NAN; r.norm = NAN; r.grad_dot_step = NAN;
      r.n_free = 0; r.status = invalid ? 2 : 1;
      rec[w] = r;
    }
    return;
  }
  const bool frame0 = gauge == VILO_COV_GAUGE_FRAME0;
  double *dxs = Rg;                                            // [96] prior dx
  short *inv_pmap = (short *)(Rg + VILO_MAX_PRIOR_DIM);        // [224] prior row of a camera dimension
  if (tid == 0) bad_s = 0;
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Pm[e] = 0.0;
  for (int e = tid; e < SS_L; e += GN_T) G[e] = 0.0;   // (Bd, Ao; every L_k and T_k that is read is written first)
  for (int e = tid; e < 143 * GN_NP; e += GN_T) BP[e] = 0.0;
  for (int e = tid; e < CD_N; e += GN_T) { bv[e] = 0.0; dsc[e] = 0.0; }
  prior_view_init(b, wm, w, b.prior_map + (size_t)w * 96, dxs, inv_pmap);

  // ---- 1. g, h and dd of the 222 state entries ----
  double g = 0.0, h = 0.0, dd = 0.0;
  bool act = false;
  const int cd = tid < GN_NS ? caller_cd(tid) : CD_N - 1;
  if (tid < GN_NS) {
    act = cd_active(cd, F, wm.const_mask);
    if (act) {
      state_entry_gh<true>(b, wm, w, cd, inv_pmap, dxs, g, h);
      if (!isfinite(g) || !isfinite(h) || h < 0.0) bad_s = 1;
      else dd = step_dd(h, lo, hi);
      bv[cd] = g;
    }
  }
  __syncthreads();   // (dxs / inv_pmap are done with: the region is the landmark staging below)

  // ---- 2. assembly ----
  assemble_visual_pose_block(b, wm, Pm);
  assemble_imu_grams(b, wm, w, Pm, Bd, Ao, BP);
  assemble_prior(b, wm, w, Pm, Bd, Ao, BP, &bad_s);
  // damping: mu D^2 / s^2 on the diagonal, by the entry's owner
  if (act) {
    if (cd < CD_B0) Pm[cd * GN_NP + cd] += mu * dd;
    else Bd[((cd - CD_B0) / 13) * 169 + ((cd - CD_B0) % 13) * 14] += mu * dd;
  }
  __syncthreads();
  // landmarks: P -= w_l w_l^T / E~_l, g_P -= w_l g_l / E~_l, ST_LMC landmarks at a time (rows scaled by E~_l^-1/2; rows up to a multiple of 4 zero)
  {
    const double *wl = b.lm_w + 80 * (size_t)wm.lm_off, *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
    double *sl = lc, *gls = lc + ST_LMC;
    for (int l0 = 0; l0 < L; l0 += ST_LMC) {
      const int nl = min(ST_LMC, L - l0), nr = (nl + 3) & ~3;
      if (tid < nl) {
        const double E = lmE[l0 + tid], gl = lmg[l0 + tid];
        double s = 0.0;
        if (!isfinite(E) || !isfinite(gl) || E < 0.0) bad_s = 1;
        else {
          const double Et = E + mu * step_dd(E, lo, hi);
          if (!(Et > 0.0) || !isfinite(Et)) bad_s = 1;
          else s = 1.0 / sqrt(Et);
        }
        sl[tid] = s;
        gls[tid] = gl * s;
      }
      __syncthreads();
      for (int e = tid; e < ST_LMC * GN_NP; e += GN_T) {
        const int li = e % ST_LMC, a = e / ST_LMC;
        if (li < nr) Rg[li * GN_NP + a] = (li < nl && a < VILO_NPU) ? wl[(size_t)a * L + l0 + li] * sl[li] : 0.0;
      }
      __syncthreads();
      step_syrk(Pm, Rg, nr / 4);
      if (tid < GN_NP) {
        double s = 0.0;
        for (int li = 0; li < nl; ++li) s += Rg[li * GN_NP + tid] * gls[li];
        bv[tid] -= s;
      }
      __syncthreads();
    }
  }

  // ---- 3. gauge: frame 0's rotation in the basis Q = [e1 e2 u], u = R0^T e_z ----
  if (frame0) {
    if (tid == 0) {
      gauge_basis(b.x + (size_t)w * XSTRIDE + XO_POSE + 3, Q);
      double r[3];
      for (int m2 = 0; m2 < 3; ++m2) r[m2] = Q[3 * m2] * bv[3] + Q[3 * m2 + 1] * bv[4] + Q[3 * m2 + 2] * bv[5];
      for (int m2 = 0; m2 < 3; ++m2) bv[3 + m2] = r[m2];
    }
    __syncthreads();
    gauge_rotate(Pm, BP, Q);
  }

  // ---- 4. equilibration; constant / absent / gauge-held dimensions: scale 0, unit diagonal, zero right-hand side ----
  for (int c = tid; c < CD_N; c += GN_T) {
    const bool on = cd_active(c, F, wm.const_mask) && !(frame0 && (c < 3 || c == 5));
    double d = 0.0;
    if (on) {
      const double hh = c < CD_B0 ? Pm[c * GN_NP + c] : Bd[((c - CD_B0) / 13) * 169 + ((c - CD_B0) % 13) * 14];
      if (!(hh > 0.0) || !isfinite(hh)) bad_s = 1;
      else d = 1.0 / sqrt(hh);
    }
    dsc[c] = d;
    bv[c] = -bv[c] * d;   // (the right-hand side of H delta = -g)
    if (d == 0.0) bv[c] = 0.0;
  }
  __syncthreads();
  scale_system(Pm, Bd, Ao, BP, dsc);
  for (int e = tid; e < ST_LMC * GN_NP; e += GN_T) Rg[e] = 0.0;   // (rows 13 .. 15 of Mg stay zero)
  __syncthreads();

  // ---- 5. forward over the chain ----
  double *yB = bv + CD_B0;
  for (int k = 0; k < VILO_F; ++k) {
    for (int e = tid; e < 169; e += GN_T) lc[e] = Bd[k * 169 + e];
    if (k > 0 && tid < 13) {   // row tid of T = A_{k,k-1} L_{k-1}^-T
      const double *a = Ao + k * 169 + tid * 13;
      double t[13];
#pragma unroll
      for (int c = 0; c < 13; ++c) {
        double s = a[c];
#pragma unroll
        for (int m = 0; m < c; ++m) s -= t[m] * lp[c * 13 + m];
        t[c] = s / lp[c * 13 + c];
      }
#pragma unroll
      for (int c = 0; c < 13; ++c) { tn[tid * 13 + c] = t[c]; Tg[k * 169 + tid * 13 + c] = t[c]; }
    }
    __syncthreads();
    if (k > 0) {
      for (int e = tid; e < 169; e += GN_T) {
        const int r = e / 13, c = e % 13;
        double s = 0.0;
        for (int m = 0; m < 13; ++m) s += tn[r * 13 + m] * tn[c * 13 + m];
        lc[e] -= s;
      }
      __syncthreads();
    }
    chol13(lc, thr, &bad_s);
    for (int e = tid; e < 169; e += GN_T) Lg[k * 169 + e] = lc[e];
    // the right-hand side z = b_k - T y_{k-1} (in place)
    if (k > 0 && tid >= GN_T - 13) {
      const int r = tid - (GN_T - 13);
      double s = yB[13 * k + r];
      for (int m = 0; m < 13; ++m) s -= tn[r * 13 + m] * yB[13 * (k - 1) + m];
      yB[13 * k + r] = s;
    }
    __syncthreads();
    // Y_k = L_k^-1 (BP_k - T Y_{k-1}), column p by thread p (Y_{k-1}'s column p read out of Mg, Y_k's written into Mg and BP_k);
    // y_k = L_k^-1 z by thread 80
    if (tid < GN_NP) {
      double y[13];
#pragma unroll
      for (int r = 0; r < 13; ++r) y[r] = BP[(size_t)(13 * k + r) * GN_NP + tid];
      if (k > 0) {
#pragma unroll 1
        for (int m = 0; m < 13; ++m) {   // (rolled: 169 hoisted loads of T would cost the second workgroup its registers)
          const double ym = Mg[m * GN_NP + tid];
#pragma unroll
          for (int r = 0; r < 13; ++r) y[r] -= tn[r * 13 + m] * ym;
        }
      }
#pragma unroll
      for (int r = 0; r < 13; ++r) {
        double s = y[r];
#pragma unroll
        for (int m = 0; m < r; ++m) s -= lc[r * 13 + m] * y[m];
        y[r] = s / lc[r * 13 + r];
      }
#pragma unroll
      for (int r = 0; r < 13; ++r) { Mg[r * GN_NP + tid] = y[r]; BP[(size_t)(13 * k + r) * GN_NP + tid] = y[r]; }
    } else if (tid == GN_NP) {
      double y[13];
#pragma unroll
      for (int r = 0; r < 13; ++r) {
        double s = yB[13 * k + r];
#pragma unroll
        for (int m = 0; m < r; ++m) s -= lc[r * 13 + m] * y[m];
        y[r] = s / lc[r * 13 + r];
      }
#pragma unroll
      for (int r = 0; r < 13; ++r) yB[13 * k + r] = y[r];
    }
    __syncthreads();
    step_syrk(Pm, Mg, 4);   // S_P -= Y_k^T Y_k
    if (tid < GN_NP) {
      double s = 0.0;
      for (int r = 0; r < 13; ++r) s += Mg[r * GN_NP + tid] * yB[13 * k + r];
      bv[tid] -= s;
    }
    for (int e = tid; e < 169; e += GN_T) lp[e] = lc[e];
    __syncthreads();
  }
  // Cholesky of S_P (lower, in place); the forward substitution of the right-hand side rides along as one more row
  for (int j = 0; j < GN_NP; ++j) {
    if (tid == 0) {
      double p = Pm[j * GN_NP + j];
      if (!(p > thr)) { bad_s = 1; p = 1.0; }
      Pm[j * GN_NP + j] = sqrt(p);
    }
    __syncthreads();
    const double piv = Pm[j * GN_NP + j];
    for (int r = j + 1 + tid; r < GN_NP; r += GN_T) Pm[r * GN_NP + j] /= piv;
    if (tid == GN_T - 1) bv[j] /= piv;
    __syncthreads();
    const int n = GN_NP - j - 1;
    for (int e = tid; e < n * n; e += GN_T) {
      const int r = j + 1 + e / n, c = j + 1 + e % n;
      if (c <= r) Pm[r * GN_NP + c] -= Pm[r * GN_NP + j] * Pm[c * GN_NP + j];
    }
    if (tid >= GN_T - GN_NP) {
      const int c = j + 1 + (tid - (GN_T - GN_NP));
      if (c < GN_NP) bv[c] -= Pm[c * GN_NP + j] * bv[j];
    }
    __syncthreads();
  }
  // L_P^T x_P = y_P: thread r keeps y_r, thread j publishes x_j
  {
    double yr = tid < GN_NP ? bv[tid] : 0.0;
    for (int j = GN_NP - 1; j >= 0; --j) {
      if (tid == j) bv[j] = yr / Pm[j * GN_NP + j];
      __syncthreads();
      if (tid < j) yr -= Pm[j * GN_NP + tid] * bv[j];
    }
    __syncthreads();
  }
  // u = y_B - Y x_P, then backward over the chain: L_k^T x_k = u_k - T_{k+1}^T x_{k+1}
  if (tid < 143) {
    const double *row = BP + (size_t)tid * GN_NP;
    double s = 0.0;
    for (int p = 0; p < GN_NP; ++p) s += row[p] * bv[p];
    yB[tid] -= s;
  }
  __syncthreads();
  for (int k = VILO_F - 1; k >= 0; --k) {
    for (int e = tid; e < 169; e += GN_T) { lc[e] = Lg[k * 169 + e]; if (k + 1 < VILO_F) tn[e] = Tg[(k + 1) * 169 + e]; }
    __syncthreads();
    double v = 0.0;
    if (tid < 13) {
      v = yB[13 * k + tid];
      if (k + 1 < VILO_F)
        for (int m = 0; m < 13; ++m) v -= tn[m * 13 + tid] * yB[13 * (k + 1) + m];
    }
    for (int j = 12; j >= 0; --j) {
      if (tid == j) yB[13 * k + j] = v / lc[j * 13 + j];
      __syncthreads();
      if (tid < j) v -= lc[j * 13 + tid] * yB[13 * k + j];
    }
    __syncthreads();
  }

  // ---- 6. the step in the caller's coordinates ----
  for (int c = tid; c < CD_N; c += GN_T) bv[c] *= dsc[c];
  __syncthreads();
  if (frame0 && tid == 0) {   // back from the basis Q (the u component is zero)
    double r[3];
    for (int i = 0; i < 3; ++i) r[i] = Q[i] * bv[3] + Q[3 + i] * bv[4] + Q[6 + i] * bv[5];
    for (int i = 0; i < 3; ++i) bv[3 + i] = r[i];
  }
  __syncthreads();
  double a_gd = 0.0, a_dd = 0.0, a_sq = 0.0;   // sums of g delta, dd delta^2, delta^2 of this thread's entries
  int a_nf = 0, a_bad = 0;
  double ds = 0.0;
  if (act) {
    ds = bv[cd];
    a_gd = g * ds; a_dd = dd * ds * ds; a_sq = ds * ds;
    a_nf = (frame0 && cd < 3) ? 0 : 1;
    if (!isfinite(ds)) a_bad = 1;
  }
  if (frame0 && tid == 0) a_nf -= 1;   // (the u direction of frame 0's rotation)
  {
    const double *wl = b.lm_w + 80 * (size_t)wm.lm_off, *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
    const int *perm = b.lm_perm + wm.lm_off;
    for (int l = tid; l < L; l += GN_T) {
      const double E = lmE[l], gl = lmg[l];
      const double ddl = (isfinite(E) && E >= 0.0) ? step_dd(E, lo, hi) : NAN;
      double s = gl;
      for (int a = 0; a < VILO_NPU; ++a) s += wl[(size_t)a * L + l] * bv[a];
      const double dl = -s / (E + mu * ddl);
      lo_out[perm[l]] = dl;
      a_gd += gl * dl; a_dd += ddl * dl * dl; a_sq += dl * dl;
      ++a_nf;
      if (!isfinite(dl)) a_bad = 1;
    }
  }

  // ---- 7. the window record ----
  double *r_gd = Rg, *r_dd = Rg + GN_T, *r_sq = Rg + 2 * GN_T;
  int *r_nf = (int *)(Rg + 3 * GN_T), *r_bad = r_nf + GN_T;
  r_gd[tid] = a_gd; r_dd[tid] = a_dd; r_sq[tid] = a_sq; r_nf[tid] = a_nf; r_bad[tid] = a_bad;
  __syncthreads();
  for (int st = GN_T / 2; st > 0; st >>= 1) {
    if (tid < st) {
      const int o = tid + st;
      r_gd[tid] += r_gd[o];
      r_dd[tid] += r_dd[o];
      r_sq[tid] += r_sq[o];
      r_nf[tid] += r_nf[o];
      r_bad[tid] |= r_bad[o];
    }
    __syncthreads();
  }
  const bool bad = bad_s != 0 || r_bad[0] != 0;
  if (tid < GN_NS) so[tid] = bad ? NAN : ds;
  if (bad)
    for (int l = tid; l < L; l += GN_T) lo_out[l] = NAN;
  if (tid == 0) {
    vilo_window_step_record r;
    const double gd = r_gd[0], sdd = r_dd[0];
    r.model_cost_change = bad ? NAN : -0.5 * gd + 0.5 * mu * sdd;
    r.scaled_norm = bad ? NAN : sqrt(sdd);
    r.norm = bad ? NAN : sqrt(r_sq[0]);
    r.grad_dot_step = bad ? NAN : gd;
    r.n_free = r_nf[0];
    r.status = bad ? 1 : 0;
    rec[w] = r;
  }
}

extern "C" void vilo_default_step_opts(vilo_step_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->gauge = VILO_COV_GAUGE_NONE;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->min_pivot = 1e-14;
}

extern "C" int vilo_set_gn_step_form(vilo_ctx *ctx, int form) {
  if (!ctx || (form != 0 && form != 1)) return VILO_ERR_BAD_ARG;
  ctx->gn_step_form = form;
  return VILO_OK;
}

extern "C" double vilo_last_gn_step_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_gn_step_ms : -1.0; }

bool vilo_step_opts_ok(const vilo_step_opts &o) {
  return (o.gauge == VILO_COV_GAUGE_FRAME0 || o.gauge == VILO_COV_GAUGE_NONE) && o.pad0 == 0 && o.min_lm_diagonal >= 0.0 &&
         o.max_lm_diagonal >= o.min_lm_diagonal && isfinite(o.max_lm_diagonal) && o.min_pivot >= 0.0 && isfinite(o.min_pivot);
}

// window records | mu | state step | landmark step | per-window scratch of one chunk
GnStepBlocks::GnStepBlocks(vilo::CallLayout &lay, const BatchDev &bd, bool has_mu_)
    : has_mu(has_mu_), chunk(std::min(bd.W, ST_CHUNK)), o_rec(lay.take<vilo_window_step_record>(bd.W)), o_mu(lay.take<double>(bd.W, has_mu_)),
      o_ss(lay.take<double>(GN_NS * (size_t)bd.W)), o_ls(lay.take<double>(bd.n_lm)), o_scr(lay.take<double>((size_t)chunk * SS_N)) {}

int vilo_gn_step_launch(vilo_ctx *ctx, BatchCall &call, const BatchDev &bd, const GnStepBlocks &gb, const vilo_step_opts &o) {
  const int W = bd.W;
  const bool resident = ctx->gn_step_form == 1;
  const size_t lds_bytes = sizeof(double) * (resident ? StepForm<true>::N : StepForm<false>::N);
  if (!ctx->step_attr_set) {
    VILO_HIP(hipFuncSetAttribute((const void *)k_gn_step<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * StepForm<false>::N)));
    VILO_HIP(hipFuncSetAttribute((const void *)k_gn_step<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * StepForm<true>::N)));
    ctx->step_attr_set = true;
  }
  for (int w0 = 0; w0 < W; w0 += gb.chunk) {
    const int n = std::min(gb.chunk, W - w0);
    hipLaunchKernelGGL(resident ? k_gn_step<true> : k_gn_step<false>, dim3(n), dim3(GN_T), lds_bytes, ctx->stream, bd, w0, o.gauge, o.min_lm_diagonal, o.max_lm_diagonal, o.min_pivot,
                       gb.has_mu ? call.ptr<double>(gb.o_mu) : (const double *)nullptr, call.ptr<double>(gb.o_scr), call.ptr<vilo_window_step_record>(gb.o_rec),
                       call.ptr<double>(gb.o_ss), call.ptr<double>(gb.o_ls));
  }
  VILO_HIP(hipGetLastError());
  return VILO_OK;
}

extern "C" int vilo_batch_gauss_newton_step(vilo_ctx *ctx, vilo_batch *bt, const vilo_step_opts *opts, const double *mu, vilo_window_step_record *windows,
                                            double *state_step, double *lm_step) {
  if (!ctx || !bt || !windows) return VILO_ERR_BAD_ARG;
  if (bt->mask.refuse(ctx, "vilo_batch_gauss_newton_step") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  vilo_step_opts o;
  if (opts) o = *opts; else vilo_default_step_opts(&o);
  if (!vilo_step_opts_ok(o)) {
    ctx->err = "vilo_batch_gauss_newton_step: bad options (gauge, pad0 == 0, 0 <= min_lm_diagonal <= max_lm_diagonal < inf, min_pivot >= 0)";
    return VILO_ERR_BAD_ARG;
  }
  BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm;
  BatchCall call(ctx, bt, &vilo_ctx::last_gn_step_ms);
  // the call's device memory: saved solver state | k_gn_step's blocks
  const size_t o_st = call.lay.take<SolverState>(W);
  const GnStepBlocks gb(call.lay, bd, mu != nullptr);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  if (mu) VILO_HIP(hipMemcpy(call.ptr<double>(gb.o_mu), mu, sizeof(double) * (size_t)W, hipMemcpyHostToDevice));
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  rc = vilo_gn_step_launch(ctx, call, bd, gb, o);
  if (rc != VILO_OK) return rc;
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  VILO_HIP(call.down(windows, call.ptr<char>(gb.o_rec), sizeof(vilo_window_step_record) * (size_t)W));
  VILO_HIP(call.down(state_step, call.ptr<char>(gb.o_ss), sizeof(double) * GN_NS * (size_t)W));
  VILO_HIP(call.down(lm_step, call.ptr<char>(gb.o_ls), sizeof(double) * (size_t)n_lm));
  return VILO_OK;
}

extern "C" int vilo_window_gauss_newton_step(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                             const vilo_step_opts *opts, const double *mu, vilo_window_step_record *windows, double *state_step,
                                             double *lm_step) {
  if (!ctx || n_windows < 1 || !in || !state || !windows) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state,
                         [&](vilo_batch *bt) { return vilo_batch_gauss_newton_step(ctx, bt, opts, mu, windows, state_step, lm_step); });
}
