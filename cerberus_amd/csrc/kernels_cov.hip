// State covariance of every window of a batch at its current device state (vilo_batch_covariance, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0: full 23-column visual rows with td, whitened IMU Grams), on the
// batch's live state x / lambda. Its first kernel re-initialises the solver state the linearisation kernels read (need_lin / done); the
// window's SolverState is saved before and copied back after, so the trust-region state, radius, mu and the summaries the next
// vilo_batch_download reports are what they were. x, xc, lambda and the prior are only read.
//
// k_covariance, one workgroup per window, all FP64. The camera-side dimensions split as the solver splits them (solver_types.hpp):
//   P  (79, LDS)      poses 6k..6k+5, ex0 66..71, ex1 72..77, td 78 (79: padding, treated as a constant dimension)
//   B  (11 x 13)      speed / bias / leg bias of frame k: block tridiagonal (the IMU factors couple consecutive frames only)
//   BP (143 x 80)     coupling of B with P (IMU factors: poses k-1, k, k+1; the prior: any pose / extrinsic / td)
// The reading of the linearisation (assembly, gauge, scaling, 13 x 13 Cholesky) is gn_system.hpp's, shared with k_gn_step. Steps:
//   1. Assemble H = J^T J without damping: visual Gram slots into P (assemble_visual_pose_block), IMU Grams (assemble_imu_grams), prior
//      (assemble_prior), the landmarks' Schur complement P -= w w^T / E.
//   2. FRAME0 gauge (gauge_basis, gauge_rotate): frame 0's rotation rows / columns in the basis [e1 e2 u] (u = R0^T e_z): the u direction and frame 0's position
//      become constant dimensions; Sigma = N (N^T H N)^-1 N^T is the inverse with those rows and columns left out.
//   3. Jacobi equilibration (unit diagonal of the reduced camera system); a constant or absent dimension gets scale 0 (its rows come out
//      zero) and a unit pivot.
//   4. Block Cholesky of the B chain (L_k^-1, T_k = A_{k,k-1} L_{k-1}^-T), Y = L_B^-1 BP, the pose system S_P = P - Y^T Y, its Cholesky
//      factor and Sigma_PP = S_P^-1. Every pivot must exceed min_reciprocal_condition.
//   5. Backward over the chain: G_k = (H_BB^-1 H_BP)_k, (H_BB^-1)_kk by the selected-inversion recursion
//      X_kk = L_k^-T L_k^-1 + V_k^T X_{k+1,k+1} V_k (V_k = T_{k+1} L_k^-1), Sigma_BB,kk = X_kk + G_k Sigma_PP G_k^T,
//      Sigma_PB,k = -Sigma_PP G_k^T; the frame's 19 x 19 block is scaled back and written.
// Scratch in global memory per window (B blocks, BP / Y / G) is per-call memory of the batch's arena; windows go through it in chunks.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>

#include "batch_call.hpp"
#include "gn_system.hpp"

static_assert(sizeof(vilo_cov_opts) == 24, "vilo_cov_opts layout (cerberus_amd/_ctypes.py mirrors it)");

#define CV_NB 13
#define CV_FR 19
#define CV_FRN (VILO_MAX_FRAMES * CV_FR * CV_FR)   // 3971 doubles of frame blocks per window
#define CV_PN (VILO_NPU * VILO_NPU)                // 6241 doubles of the pose system per window
#define CV_CHUNK 4096       // windows per scratch pass
// global scratch per window (doubles)
#define CS_BD 0                              // [11][13][13] diagonal blocks of B
#define CS_AO (CS_BD + 11 * 169)             // [11][13][13] A_{k,k-1} (row: frame k, column: frame k - 1), k >= 1
#define CS_LI (CS_AO + 11 * 169)             // [11][13][13] L_k^-1
#define CS_T (CS_LI + 11 * 169)              // [11][13][13] T_k = A_{k,k-1} L_{k-1}^-T
#define CS_BP (CS_T + 11 * 169)              // [143][80] BP, then Y, then G
#define CS_N (CS_BP + 143 * GN_NP)
// LDS (doubles)
#define CL_P 0                               // [80][80] pose system, then Sigma_PP (scaled)
#define CL_S (CL_P + GN_NP * GN_NP)          // [80][80] landmark staging / L_P^-1 / output staging
#define CL_Z (CL_S + GN_NP * GN_NP)          // [13][80]
#define CL_M (CL_Z + CV_NB * GN_NP)          // [13][80]
#define CL_SM (CL_M + CV_NB * GN_NP)         // six 13 x 13: ss, lc, lp, tn, vs, xs
#define CL_D (CL_SM + 6 * 169)               // [224] scale of every camera dimension (0: constant / absent)
#define CL_Q (CL_D + CD_N)                   // [9] Q = [e1 e2 u] (column-major: Q[3 m + i] = i-th entry of column m)
#define CL_N (CL_Q + 16)
#define CL_LMC 64                            // landmarks per staging pass (64 x 80 <= 6400)

// pose-system dimension p of frame k's position / rotation, or of the extrinsics / td
__device__ __forceinline__ bool cov_active(int cd, const WinMeta &wm, int gauge) {
  if (cd < CD_B0) {
    if (cd < 66) { const int k = cd / 6; if (k >= wm.n_frames) return false; return !(gauge == VILO_COV_GAUGE_FRAME0 && cd < 3); }
    if (cd < CD_TD) return !(wm.const_mask & CONST_EX);
    if (cd == CD_TD) return !(wm.const_mask & CONST_TD);
    return false;
  }
  const int k = (cd - CD_B0) / CV_NB, c = (cd - CD_B0) % CV_NB;
  if (k >= wm.n_frames || k >= VILO_F) return false;
  if (c >= 9) return wm.use_leg && !(wm.const_mask & CONST_LB);
  return true;
}

// in-place Cholesky of the 13 x 13 block ss (chol13, gn_system.hpp), then li = L^-1 (lower, upper zeroed). *bad when a pivot <= thr.
__device__ __forceinline__ void cov_chol13(double *ss, double *li, double thr, int *bad) {
  const int tid = threadIdx.x;
  chol13(ss, thr, bad);
  if (tid < CV_NB) {
    const int c = tid;
    for (int r = 0; r < c; ++r) li[r * 13 + c] = 0.0;
    for (int r = c; r < CV_NB; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int m = c; m < r; ++m) s -= ss[r * 13 + m] * li[m * 13 + c];
      li[r * 13 + c] = s / ss[r * 13 + r];
    }
  }
  __syncthreads();
}

__global__ void __launch_bounds__(GN_T) k_covariance(BatchDev b, int w0, int gauge, double thr, int want_poses, double *scr, double *frames_out,
                                                    double *poses_out, int *status_out) {
  extern __shared__ double lds[];
  __shared__ int bad_s;
  const int w = w0 + blockIdx.x, tid = threadIdx.x;
  const WinMeta wm = b.win[w];
  double *Pm = lds + CL_P, *Sg = lds + CL_S, *Z = lds + CL_Z, *Mg = lds + CL_M, *dsc = lds + CL_D, *Q = lds + CL_Q;
  double *ss = lds + CL_SM, *lc = ss + 169, *lp = lc + 169, *tn = lp + 169, *vs = tn + 169, *xs = vs + 169;
  double *G = scr + (size_t)blockIdx.x * CS_N;
  double *Bd = G + CS_BD, *Ao = G + CS_AO, *Li = G + CS_LI, *Tg = G + CS_T, *BP = G + CS_BP;
  double *fo = frames_out + (size_t)w * CV_FRN;
  double *po = want_poses ? poses_out + (size_t)w * CV_PN : nullptr;
  const bool invalid = b.win_bad && b.win_bad[w];
  if (tid == 0) bad_s = 0;
  if (invalid) {   // a preintegration covariance without sqrt_info: the window is not linearised (k_init_state marks it done)
    for (int e = tid; e < CV_FRN; e += GN_T) fo[e] = NAN;
    if (po) for (int e = tid; e < CV_PN; e += GN_T) po[e] = NAN;
    if (tid == 0) status_out[w] = 2;
    return;
  }
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Pm[e] = 0.0;
  for (int e = tid; e < CS_N; e += GN_T) G[e] = 0.0;
  __syncthreads();

  // ---- 1. assembly ----
  assemble_visual_pose_block(b, wm, Pm);
  assemble_imu_grams(b, wm, w, Pm, Bd, Ao, BP);
  assemble_prior(b, wm, w, Pm, Bd, Ao, BP, &bad_s);
  // landmarks: P -= w_l w_l^T / E_l, the coupling rows staged CL_LMC landmarks at a time (scaled by E_l^-1/2)
  {
    const double *wl = b.lm_w + 80 * (size_t)wm.lm_off;
    for (int l0 = 0; l0 < wm.L; l0 += CL_LMC) {
      const int nl = min(CL_LMC, wm.L - l0);
      for (int e = tid; e < nl * GN_NP; e += GN_T) {
        const int li = e / GN_NP, a = e % GN_NP;
        const double E = b.lm_E[wm.lm_off + l0 + li];
        if (a == 0 && !(E > 0.0)) bad_s = 1;
        Sg[li * GN_NP + a] = (a < VILO_NPU) ? wl[(size_t)a * wm.L + l0 + li] / sqrt(E) : 0.0;
      }
      __syncthreads();
      for (int e = tid; e < GN_NP * GN_NP; e += GN_T) {
        const int i = e / GN_NP, j = e % GN_NP;
        double s = 0.0;
        for (int li = 0; li < nl; ++li) s += Sg[li * GN_NP + i] * Sg[li * GN_NP + j];
        Pm[e] -= s;
      }
      __syncthreads();
    }
  }

  // ---- 2. gauge: frame 0's rotation in the basis Q = [e1 e2 u], u = R0^T e_z ----
  const bool frame0 = gauge == VILO_COV_GAUGE_FRAME0;
  if (frame0) {
    if (tid == 0) gauge_basis(b.x + (size_t)w * XSTRIDE + XO_POSE + 3, Q);
    __syncthreads();
    gauge_rotate(Pm, BP, Q);
  }

  // ---- 3. equilibration; constant / absent dimensions: scale 0, unit diagonal ----
  for (int cd = tid; cd < CD_N; cd += GN_T) {
    bool act = cov_active(cd, wm, gauge) && !(frame0 && cd == 5);
    double d = 0.0;
    if (act) {
      const double h = cd < CD_B0 ? Pm[cd * GN_NP + cd] : Bd[((cd - CD_B0) / 13) * 169 + ((cd - CD_B0) % 13) * 14];
      if (!(h > 0.0) || !isfinite(h)) bad_s = 1;
      else d = 1.0 / sqrt(h);
    }
    dsc[cd] = d;
  }
  __syncthreads();
  scale_system(Pm, Bd, Ao, BP, dsc);
  __syncthreads();

  // ---- 4. forward over the chain: L_k^-1, T_k, Y_k; S_P = P - sum Y_k^T Y_k ----
  for (int k = 0; k < VILO_F; ++k) {
    for (int e = tid; e < 169; e += GN_T) ss[e] = Bd[k * 169 + e];
    __syncthreads();
    if (k > 0) {
      for (int e = tid; e < 169; e += GN_T) {   // T = A_{k,k-1} L_{k-1}^-T
        const int r = e / 13, c = e % 13;
        double s = 0.0;
        for (int m = 0; m <= c; ++m) s += Ao[k * 169 + r * 13 + m] * lp[c * 13 + m];
        tn[e] = s;
        Tg[k * 169 + e] = s;
      }
      __syncthreads();
      for (int e = tid; e < 169; e += GN_T) {
        const int r = e / 13, c = e % 13;
        double s = 0.0;
        for (int m = 0; m < 13; ++m) s += tn[r * 13 + m] * tn[c * 13 + m];
        ss[e] -= s;
      }
      __syncthreads();
    }
    cov_chol13(ss, lc, thr, &bad_s);
    for (int e = tid; e < 169; e += GN_T) Li[k * 169 + e] = lc[e];
    // Z = BP_k - T Y_{k-1};  Y_k = L_k^-1 Z (into BP_k and Mg)
    for (int e = tid; e < CV_NB * GN_NP; e += GN_T) {
      const int r = e / GN_NP, p = e % GN_NP;
      double s = BP[(size_t)(13 * k + r) * GN_NP + p];
      if (k > 0)
        for (int m = 0; m < 13; ++m) s -= tn[r * 13 + m] * Mg[m * GN_NP + p];
      Z[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < CV_NB * GN_NP; e += GN_T) {
      const int r = e / GN_NP, p = e % GN_NP;
      double s = 0.0;
      for (int m = 0; m <= r; ++m) s += lc[r * 13 + m] * Z[m * GN_NP + p];
      Mg[e] = s;
      BP[(size_t)(13 * k + r) * GN_NP + p] = s;
    }
    __syncthreads();
    for (int e = tid; e < GN_NP * GN_NP; e += GN_T) {
      const int i = e / GN_NP, j = e % GN_NP;
      double s = 0.0;
      for (int r = 0; r < 13; ++r) s += Mg[r * GN_NP + i] * Mg[r * GN_NP + j];
      Pm[e] -= s;
    }
    for (int e = tid; e < 169; e += GN_T) lp[e] = lc[e];
    __syncthreads();
  }
  // Cholesky of S_P (lower, in place), L_P^-1 into Sg, Sigma_PP = L_P^-T L_P^-1 into Pm
  for (int j = 0; j < GN_NP; ++j) {
    if (tid == 0) {
      double p = Pm[j * GN_NP + j];
      if (!(p > thr)) { bad_s = 1; p = 1.0; }
      Pm[j * GN_NP + j] = sqrt(p);
    }
    __syncthreads();
    const double piv = Pm[j * GN_NP + j];
    for (int r = j + 1 + tid; r < GN_NP; r += GN_T) Pm[r * GN_NP + j] /= piv;
    __syncthreads();
    const int n = GN_NP - j - 1;
    for (int e = tid; e < n * n; e += GN_T) {
      const int r = j + 1 + e / n, c = j + 1 + e % n;
      if (c <= r) Pm[r * GN_NP + c] -= Pm[r * GN_NP + j] * Pm[c * GN_NP + j];
    }
    __syncthreads();
  }
  if (tid < GN_NP) {
    const int c = tid;
    for (int r = 0; r < c; ++r) Sg[r * GN_NP + c] = 0.0;
    for (int r = c; r < GN_NP; ++r) {
      double s = (r == c) ? 1.0 : 0.0;
      for (int m = c; m < r; ++m) s -= Pm[r * GN_NP + m] * Sg[m * GN_NP + c];
      Sg[r * GN_NP + c] = s / Pm[r * GN_NP + r];
    }
  }
  __syncthreads();
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) {
    const int i = e / GN_NP, j = e % GN_NP;
    double s = 0.0;
    for (int m = max(i, j); m < GN_NP; ++m) s += Sg[m * GN_NP + i] * Sg[m * GN_NP + j];
    Pm[e] = s;
  }
  __syncthreads();
  const bool bad = bad_s != 0;

  // ---- 5. backward over the chain: G_k, X_kk, the frame blocks ----
  for (int k = VILO_F - 1; k >= 0; --k) {
    for (int e = tid; e < 169; e += GN_T) { lc[e] = Li[k * 169 + e]; if (k + 1 < VILO_F) tn[e] = Tg[(k + 1) * 169 + e]; }
    __syncthreads();
    // Z = Y_k - T_{k+1}^T G_{k+1}  (G_{k+1} in Mg)
    for (int e = tid; e < CV_NB * GN_NP; e += GN_T) {
      const int r = e / GN_NP, p = e % GN_NP;
      double s = BP[(size_t)(13 * k + r) * GN_NP + p];
      if (k + 1 < VILO_F)
        for (int m = 0; m < 13; ++m) s -= tn[m * 13 + r] * Mg[m * GN_NP + p];
      Z[e] = s;
    }
    // X_kk: V = T_{k+1} L_k^-1, X = L_k^-T L_k^-1 + V^T X_{k+1} V
    if (k + 1 < VILO_F)
      for (int e = tid; e < 169; e += GN_T) {
        const int r = e / 13, c = e % 13;
        double s = 0.0;
        for (int m = c; m < 13; ++m) s += tn[r * 13 + m] * lc[m * 13 + c];
        vs[e] = s;
      }
    __syncthreads();
    // G_k = L_k^-T Z  (into Mg);  ss = V^T X_{k+1}
    for (int e = tid; e < CV_NB * GN_NP; e += GN_T) {
      const int r = e / GN_NP, p = e % GN_NP;
      double s = 0.0;
      for (int m = r; m < 13; ++m) s += lc[m * 13 + r] * Z[m * GN_NP + p];
      Mg[e] = s;
    }
    if (k + 1 < VILO_F)
      for (int e = tid; e < 169; e += GN_T) {
        const int r = e / 13, c = e % 13;
        double s = 0.0;
        for (int m = 0; m < 13; ++m) s += vs[m * 13 + r] * xs[m * 13 + c];
        ss[e] = s;
      }
    __syncthreads();
    for (int e = tid; e < 169; e += GN_T) {
      const int r = e / 13, c = e % 13;
      double s = 0.0;
      for (int m = max(r, c); m < 13; ++m) s += lc[m * 13 + r] * lc[m * 13 + c];
      if (k + 1 < VILO_F)
        for (int m = 0; m < 13; ++m) s += ss[r * 13 + m] * vs[m * 13 + c];
      lp[e] = s;
    }
    // Z = G_k Sigma_PP
    for (int e = tid; e < CV_NB * GN_NP; e += GN_T) {
      const int r = e / GN_NP, p = e % GN_NP;
      double s = 0.0;
      for (int q = 0; q < GN_NP; ++q) s += Mg[r * GN_NP + q] * Pm[q * GN_NP + p];
      Z[e] = s;
    }
    __syncthreads();
    for (int e = tid; e < 169; e += GN_T) xs[e] = lp[e];
    __syncthreads();
    // frame block (scaled) into Sg[0 .. 361): [dp dtheta | v ba bg rho]
    for (int e = tid; e < CV_FR * CV_FR; e += GN_T) {
      const int a = e / CV_FR, c = e % CV_FR;
      double v;
      if (a < 6 && c < 6) v = Pm[(6 * k + a) * GN_NP + 6 * k + c];
      else if (a < 6) v = -Z[(c - 6) * GN_NP + 6 * k + a];
      else if (c < 6) v = -Z[(a - 6) * GN_NP + 6 * k + c];
      else {
        double s = xs[(a - 6) * 13 + (c - 6)];
        for (int p = 0; p < GN_NP; ++p) s += Z[(a - 6) * GN_NP + p] * Mg[(c - 6) * GN_NP + p];
        v = s;
      }
      const int ca = a < 6 ? 6 * k + a : CD_B0 + 13 * k + (a - 6), cc = c < 6 ? 6 * k + c : CD_B0 + 13 * k + (c - 6);
      Sg[e] = v * dsc[ca] * dsc[cc];
    }
    __syncthreads();
    if (frame0 && k == 0) {   // back from the basis Q: rows, then columns 3..5
      if (tid < CV_FR) {
        double r[3];
        for (int i = 0; i < 3; ++i) r[i] = Q[i] * Sg[3 * CV_FR + tid] + Q[3 + i] * Sg[4 * CV_FR + tid] + Q[6 + i] * Sg[5 * CV_FR + tid];
        for (int i = 0; i < 3; ++i) Sg[(3 + i) * CV_FR + tid] = r[i];
      }
      __syncthreads();
      if (tid < CV_FR) {
        double r[3];
        for (int i = 0; i < 3; ++i) r[i] = Q[i] * Sg[tid * CV_FR + 3] + Q[3 + i] * Sg[tid * CV_FR + 4] + Q[6 + i] * Sg[tid * CV_FR + 5];
        for (int i = 0; i < 3; ++i) Sg[tid * CV_FR + 3 + i] = r[i];
      }
      __syncthreads();
    }
    for (int e = tid; e < CV_FR * CV_FR; e += GN_T) {   // (symmetric to the bit: the two triangles went through different rounding)
      const int a = e / CV_FR, c = e % CV_FR;
      fo[k * CV_FR * CV_FR + e] = bad ? NAN : 0.5 * (Sg[e] + Sg[c * CV_FR + a]);
    }
    __syncthreads();
  }
  if (po) {
    for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Sg[e] = Pm[e] * dsc[e / GN_NP] * dsc[e % GN_NP];
    __syncthreads();
    if (frame0) {
      if (tid < GN_NP) {
        double r[3];
        for (int i = 0; i < 3; ++i) r[i] = Q[i] * Sg[3 * GN_NP + tid] + Q[3 + i] * Sg[4 * GN_NP + tid] + Q[6 + i] * Sg[5 * GN_NP + tid];
        for (int i = 0; i < 3; ++i) Sg[(3 + i) * GN_NP + tid] = r[i];
      }
      __syncthreads();
      if (tid < GN_NP) {
        double r[3];
        for (int i = 0; i < 3; ++i) r[i] = Q[i] * Sg[tid * GN_NP + 3] + Q[3 + i] * Sg[tid * GN_NP + 4] + Q[6 + i] * Sg[tid * GN_NP + 5];
        for (int i = 0; i < 3; ++i) Sg[tid * GN_NP + 3 + i] = r[i];
      }
      __syncthreads();
    }
    for (int e = tid; e < CV_PN; e += GN_T) {
      const int a = e / VILO_NPU, c = e % VILO_NPU;
      po[e] = bad ? NAN : 0.5 * (Sg[a * GN_NP + c] + Sg[c * GN_NP + a]);
    }
  }
  if (tid == 0) status_out[w] = bad ? 1 : 0;
}

extern "C" void vilo_default_cov_opts(vilo_cov_opts *o) {
  if (!o) return;
  memset(o, 0, sizeof(*o));
  o->gauge = VILO_COV_GAUGE_FRAME0;
  o->min_reciprocal_condition = 1e-14;
  o->want_poses = 0;
}

extern "C" double vilo_last_covariance_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_cov_ms : -1.0; }

// ---- landmark covariance (vilo_batch_landmark_covariance, include/vilo_gpu.h) ----
// Landmarks couple only to the pose system, so with Sigma_PP (k_covariance's `poses` output: unscaled, original basis, symmetric to the
// bit) and the mode-0 linearisation's E_l (lm_E) and w_l (lm_w, [80][L] per window):
//   Sigma_rr = 1 / E + w^T Sigma_PP w / E^2,  Sigma_rP = -w^T Sigma_PP / E.
// k_landmark_covariance, one workgroup of four waves per window: Sigma_PP in LDS (80 x 80, row / column 79 zero). Each wave takes 16
// landmarks at a time and forms U = Sigma_PP W (80 x 16) as five 16 x 16 FP64-MFMA tiles over 20 k-steps (100 MFMAs). The B operand of
// k-step ks, W[4 ks + lk][lr], is also W at the accumulator position (row 16 X + lk + 4 r: ks = 4 X + r), so w^T U comes from the
// registers and a reduction over the four 16-lane groups. The 12 entries of U at pose s and ex0 go through LDS to one lane per landmark,
// which forms the joint covariance of [dp_s dtheta_s dt_c dtheta_c rho], the world point p = R_s (R_c f / rho + t_c) + P_s and
// Sigma_p = J Sigma_13 J^T.
#define LC_T 256
#define LC_S 0                        // [80][80] Sigma_PP
#define LC_U (LC_S + GN_NP * GN_NP)   // [4 waves][16][12] U at pose s (dp dtheta) and ex0 (dt dtheta)
#define LC_N (LC_U + 4 * 16 * 12)     // 57 344 bytes: two workgroups per CU

// pp: Sigma_PP of window w0 + blockIdx.x at pp + blockIdx.x * 6241; status: k_covariance's, by window. Outputs in the caller's landmark
// order (wm.lm_off + lm_perm).
__global__ void __launch_bounds__(LC_T) k_landmark_covariance(BatchDev b, int w0, const double *pp, const int *status, double *var_out,
                                                             double *pts_out, double *pcov_out) {
  using namespace vilo;
  extern __shared__ double lds[];
  const int w = w0 + blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const WinMeta wm = b.win[w];
  if (wm.L == 0) return;
  if (status[w] != 0) {
    for (int l = tid; l < wm.L; l += LC_T) {
      const int o = wm.lm_off + b.lm_perm[wm.lm_off + l];
      var_out[o] = NAN;
      for (int c = 0; c < 3; ++c) pts_out[3 * (size_t)o + c] = NAN;
      for (int c = 0; c < 9; ++c) pcov_out[9 * (size_t)o + c] = NAN;
    }
    return;
  }
  double *S = lds + LC_S, *Uw = lds + LC_U + wave * 16 * 12;
  const double *src = pp + (size_t)blockIdx.x * CV_PN;
  for (int e = tid; e < GN_NP * GN_NP; e += LC_T) {
    const int i = e / GN_NP, j = e % GN_NP;
    S[e] = (i < VILO_NPU && j < VILO_NPU) ? src[i * VILO_NPU + j] : 0.0;
  }
  __syncthreads();
  const double *wl = b.lm_w + 80 * (size_t)wm.lm_off;
  const double *xw = b.x + (size_t)w * XSTRIDE;
  for (int l0 = 0; l0 < wm.L; l0 += 64) {
    const int lw0 = l0 + 16 * wave, l = lw0 + lr;   // this lane's landmark (window-local device order)
    const bool act = lw0 < wm.L, on = l < wm.L;     // (act: wave-uniform)
    const int s = on ? b.lm_s[wm.lm_off + l] : 0;
    double q = 0.0;
    if (act) {
      double B[20];
#pragma unroll
      for (int ks = 0; ks < 20; ++ks) {
        const int k = 4 * ks + lk;
        B[ks] = (on && k < VILO_NPU) ? wl[(size_t)k * wm.L + l] : 0.0;
      }
      mfma_d4 U[5];
#pragma unroll
      for (int X = 0; X < 5; ++X) U[X] = mfma_d4{0.0, 0.0, 0.0, 0.0};
      // A[row 16 X + lr][k 4 ks + lk] = Sigma_PP[4 ks + lk][16 X + lr] (symmetric): 16 consecutive doubles per lane group
#pragma unroll
      for (int ks = 0; ks < 20; ++ks)
#pragma unroll
        for (int X = 0; X < 5; ++X) U[X] = __builtin_amdgcn_mfma_f64_16x16x4f64(S[(4 * ks + lk) * GN_NP + 16 * X + lr], B[ks], U[X], 0, 0, 0);
#pragma unroll
      for (int X = 0; X < 5; ++X)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          q += U[X][r] * B[4 * X + r];
          const int row = 16 * X + lk + 4 * r;
          const int j = (row >= 6 * s && row < 6 * s + 6) ? row - 6 * s : ((row >= CD_EX0 && row < CD_EX0 + 6) ? 6 + row - CD_EX0 : -1);
          if (j >= 0) Uw[lr * 12 + j] = U[X][r];
        }
      q += __shfl_xor(q, 16);
      q += __shfl_xor(q, 32);
    }
    __syncthreads();
    if (on && lk == 0) {
      const int gi = wm.lm_off + l, o = wm.lm_off + b.lm_perm[gi];
      const double Ei = 1.0 / b.lm_E[gi], vr = Ei + q * Ei * Ei;
      // first observation: the packed wave and lane of device landmark l (the left point of t = 0 in the wave's image)
      double f[3] = {0.0, 0.0, 0.0};
      for (int wi = wm.wave_off; wi < wm.wave_off + wm.n_waves; ++wi) {
        const WaveMeta wv = b.wave[wi];
        for (int g = 0; g < wv.nseg; ++g) {
          const ChunkMeta cm = b.chunk[wv.seg_chunk[g]];
          const int i = l - cm.lm_local;
          if (i >= 0 && i < cm.n) {
            for (int c = 0; c < 3; ++c) f[c] = obs_at(b.obs + wv.obs_off, wv.n_lanes, wv.seg_lane0[g] + i, 0, OBS_LX + c);
          }
        }
      }
      const double ir = 1.0 / b.lam[gi];
      const m3 Rs = qR(qnormalized(ldq_pose(xw + XO_POSE + 7 * s))), Rc = qR(qnormalized(ldq_pose(xw + XO_EX)));
      const v3 fv = mk3(f[0], f[1], f[2]), a = fv * ir, bc = Rc * a + ld3(xw + XO_EX);
      const v3 p = Rs * bc + ld3(xw + XO_POSE + 7 * s);
      const m3 Dth = -(Rs * skew(bc)), RsRc = Rs * Rc, Dthc = -(RsRc * skew(a));
      const v3 Dr = -(RsRc * fv) * (ir * ir);
      // J = [JP | Dr] over [dp_s dtheta_s dt_c dtheta_c | rho];  Sigma_13 = [[S12, c], [c^T, vr]], c = -U12 / E
      double JP[3][12], cv[12], D[3] = {Dr.x, Dr.y, Dr.z};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          JP[r][c] = r == c ? 1.0 : 0.0;
          JP[r][3 + c] = Dth(r, c);
          JP[r][6 + c] = Rs(r, c);
          JP[r][9 + c] = Dthc(r, c);
        }
#pragma unroll
      for (int j = 0; j < 12; ++j) cv[j] = -Uw[lr * 12 + j] * Ei;
      double R[3][3];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double T[12], Jc = 0.0;   // T = (JP S12)_r
#pragma unroll
        for (int j = 0; j < 12; ++j) {
          const int dj = j < 6 ? 6 * s + j : CD_EX0 + j - 6;
          double t = 0.0;
#pragma unroll
          for (int m = 0; m < 12; ++m) t += JP[r][m] * S[(m < 6 ? 6 * s + m : CD_EX0 + m - 6) * GN_NP + dj];
          T[j] = t;
          Jc += JP[r][j] * cv[j];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          double t = 0.0, Jcc = 0.0;
#pragma unroll
          for (int j = 0; j < 12; ++j) { t += T[j] * JP[c][j]; Jcc += JP[c][j] * cv[j]; }
          R[r][c] = t + Jc * D[c] + D[r] * Jcc + vr * D[r] * D[c];
        }
      }
      var_out[o] = vr;
      st3(pts_out + 3 * (size_t)o, p);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) pcov_out[9 * (size_t)o + 3 * r + c] = 0.5 * (R[r][c] + R[c][r]);
    }
    __syncthreads();
  }
}

// vilo_batch_covariance and vilo_batch_landmark_covariance's arguments: false if the options are bad
static bool cov_opts(const vilo_cov_opts *opts, vilo_cov_opts *o) {
  if (opts) *o = *opts; else vilo_default_cov_opts(o);
  return (o->gauge == VILO_COV_GAUGE_FRAME0 || o->gauge == VILO_COV_GAUGE_NONE) && o->min_reciprocal_condition >= 0.0 && isfinite(o->min_reciprocal_condition);
}

// k_covariance indexes frames / poses by the window's index in the batch: a buffer of one chunk is handed to it shifted back by w0 windows
static double *cov_chunk_view(char *p, int w0, size_t per_window) { return (double *)((uintptr_t)p - (uintptr_t)w0 * per_window * sizeof(double)); }

// The body of vilo_batch_covariance and vilo_batch_landmark_covariance, arguments checked. want_poses: what k_covariance is told;
// frames / poses: the caller's outputs, or null to keep them in a buffer of one chunk (poses: only where want_poses); lm: the landmark
// outputs (inverse-depth variance, point, point covariance) of k_landmark_covariance after each chunk, or null for no landmark pass.
static int batch_covariance(vilo_ctx *ctx, vilo_batch *bt, const vilo_cov_opts &o, int want_poses, double *frames, double *poses, double *const *lm,
                            int32_t *status) {
  BatchDev &bd = bt->d;
  const int W = bd.W, chunk = std::min(W, CV_CHUNK);
  const size_t n_lm = lm ? (size_t)bd.n_lm : 0;
  // the call's device memory: saved solver state | frames | poses | status | per-window scratch of one chunk | landmark variance, point, point covariance
  const size_t n_fr = frames ? (size_t)W : (size_t)chunk, n_po = !want_poses ? 0 : poses ? (size_t)W : (size_t)chunk;
  BatchCall call(ctx, bt, &vilo_ctx::last_cov_ms);
  const size_t o_st = call.lay.take<SolverState>(W), o_fr = call.lay.take<double>(n_fr * CV_FRN), o_po = call.lay.take<double>(n_po * CV_PN);
  const size_t o_stat = call.lay.take<int>(W), o_scr = call.lay.take<double>((size_t)chunk * CS_N);
  const size_t o_var = call.lay.take<double>(n_lm), o_pts = call.lay.take<double>(3 * n_lm), o_pcov = call.lay.take<double>(9 * n_lm);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  double *d_var = call.ptr<double>(o_var), *d_pts = call.ptr<double>(o_pts), *d_pcov = call.ptr<double>(o_pcov);
  int *d_stat = call.ptr<int>(o_stat);
  const size_t lds_bytes = sizeof(double) * CL_N;
  if (!ctx->cov_attr_set) {
    VILO_HIP(hipFuncSetAttribute((const void *)k_covariance, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
    ctx->cov_attr_set = true;
  }
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  const int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  for (int w0 = 0; w0 < W; w0 += chunk) {
    const int n = std::min(chunk, W - w0);
    double *fr = frames ? call.ptr<double>(o_fr) : cov_chunk_view(call.ptr<char>(o_fr), w0, CV_FRN);
    double *po = poses ? call.ptr<double>(o_po) : want_poses ? cov_chunk_view(call.ptr<char>(o_po), w0, CV_PN) : nullptr;
    hipLaunchKernelGGL(k_covariance, dim3(n), dim3(GN_T), lds_bytes, ctx->stream, bd, w0, o.gauge, o.min_reciprocal_condition, want_poses,
                       call.ptr<double>(o_scr), fr, po, d_stat);
    if (lm)
      hipLaunchKernelGGL(k_landmark_covariance, dim3(n), dim3(LC_T), sizeof(double) * LC_N, ctx->stream, bd, w0, po + (size_t)w0 * CV_PN,
                         d_stat, d_var, d_pts, d_pcov);
  }
  VILO_HIP(hipGetLastError());
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  VILO_HIP(call.down(frames, call.ptr<char>(o_fr), sizeof(double) * (size_t)W * CV_FRN));
  VILO_HIP(call.down(poses, call.ptr<char>(o_po), sizeof(double) * (size_t)W * CV_PN));
  VILO_HIP(call.down(status, d_stat, sizeof(int) * (size_t)W));
  if (n_lm > 0) {
    VILO_HIP(call.down(lm[0], d_var, sizeof(double) * n_lm));
    VILO_HIP(call.down(lm[1], d_pts, sizeof(double) * 3 * n_lm));
    VILO_HIP(call.down(lm[2], d_pcov, sizeof(double) * 9 * n_lm));
  }
  return VILO_OK;
}

extern "C" int vilo_batch_covariance(vilo_ctx *ctx, vilo_batch *bt, const vilo_cov_opts *opts, double *frames, double *poses, int32_t *status) {
  if (!ctx || !bt || !frames || !status) return VILO_ERR_BAD_ARG;
  if (bt->mask.refuse(ctx, "vilo_batch_covariance") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  vilo_cov_opts o;
  if (!cov_opts(opts, &o) || (o.want_poses && !poses)) {
    ctx->err = "vilo_batch_covariance: bad options (gauge, min_reciprocal_condition >= 0, want_poses needs a poses buffer)";
    return VILO_ERR_BAD_ARG;
  }
  return batch_covariance(ctx, bt, o, o.want_poses ? 1 : 0, frames, o.want_poses ? poses : nullptr, nullptr, status);
}

extern "C" int vilo_window_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, const vilo_cov_opts *opts,
                                      double *frames, double *poses, int32_t *status) {
  if (!ctx || n_windows <= 0 || !in || !state || !frames || !status) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) { return vilo_batch_covariance(ctx, bt, opts, frames, poses, status); });
}

extern "C" int vilo_batch_landmark_covariance(vilo_ctx *ctx, vilo_batch *bt, const vilo_cov_opts *opts, double *frames, double *poses, double *inv_depth_var,
                                              double *points, double *point_cov, int32_t *status) {
  if (!ctx || !bt || !status) return VILO_ERR_BAD_ARG;
  if (bt->mask.refuse(ctx, "vilo_batch_landmark_covariance") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  vilo_cov_opts o;
  if (!cov_opts(opts, &o) || (bt->d.n_lm > 0 && (!inv_depth_var || !points || !point_cov))) {
    ctx->err = "vilo_batch_landmark_covariance: bad arguments (gauge, min_reciprocal_condition >= 0, landmark output buffers)";
    return VILO_ERR_BAD_ARG;
  }
  double *const lm[3] = {inv_depth_var, points, point_cov};
  return batch_covariance(ctx, bt, o, 1, frames, poses, lm, status);
}

extern "C" int vilo_window_landmark_covariance(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                               const vilo_cov_opts *opts, double *frames, double *poses, double *inv_depth_var, double *points,
                                               double *point_cov, int32_t *status) {
  if (!ctx || n_windows <= 0 || !in || !state || !status) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_landmark_covariance(ctx, bt, opts, frames, poses, inv_depth_var, points, point_cov, status);
  });
}
