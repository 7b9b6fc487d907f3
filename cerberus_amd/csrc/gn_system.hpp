// The one reader of what vilo_marg_linearize (mode 0) leaves behind — visual Gram slots, IMU Grams, the prior, lm_w / lm_E / lm_gbuf — for
// the query kernels that run one workgroup of GN_T threads per window: k_covariance, k_gradient, k_gn_step, k_hess_vec, k_dogleg. Every piece is
// defined here once; a change of the Gram slot layout, of the prior_map convention or of the gauge is made here and nowhere else.
//   caller_cd              caller layout (222 entries) -> camera dimension                   gradient, step, Hessian-vector
//   prior_view_init        prior dx and the inverse of prior_map                             gradient, step, Hessian-vector
//   state_entry_gh         g (and h) of one state entry, by its owner                        gradient, step, Hessian-vector (g only)
//   assemble_visual_pose_block   visual Gram slots -> the 80 x 80 pose block P               covariance, step, Hessian-vector
//   assemble_imu_grams, assemble_prior   IMU Grams / the prior's H -> P, Bd, Ao, BP          covariance, step
//   gauge_basis, gauge_rotate    FRAME0 gauge: Q = [e1 e2 u] and H' = Q^T H Q                covariance, step
//   scale_system           Jacobi scaling of P, Bd, Ao, BP                                   covariance, step
//   chol13                 in-place Cholesky of a 13 x 13 block                              covariance, step
//   step_dd                D^2 / s^2 of a coordinate from its Gauss-Newton diagonal          step, dogleg
//   hv_imu_cd, hv_tile     an IMU Gram's camera dimensions; one 16 x 16 matrix-core tile     Hessian-vector, dogleg
// The camera-side dimensions split as the solver splits them (solver_types.hpp):
//   P  (79 + 1 padding, row stride GN_NP)   poses 6k..6k+5, ex0 66..71, ex1 72..77, td 78
//   Bd / Ao ([11][13][13] each)             diagonal blocks of the speed / bias / leg-bias chain and A_{k,k-1} (row: frame k, column: frame k - 1)
//   BP ([143][GN_NP])                       coupling of the chain with P
// Every function is called by all GN_T threads of the workgroup unless it says otherwise; the ones that contain barriers say so. The order of
// every sum is fixed (owner-computes or one target per thread and barrier interval): no floating-point atomics.
#pragma once
#include "batch_state.hpp"
#include "cost_eval.hpp"
#include "solve_common.hpp"
#include "vilo_math.hpp"

#define GN_T 256    // threads per window
#define GN_NP 80    // row stride of the pose system
#define GN_NS 222   // state entries per window (VILO_NCAM)

// camera dimension (solver_types.hpp) of entry d of the caller's layout (pose 11 x 6, speed-bias 11 x 9, leg bias 11 x 4, extrinsics 2 x 6, td)
__device__ __forceinline__ int caller_cd(int d) {
  if (d < 66) return d;
  if (d < 165) { const int k = (d - 66) / 9; return CD_B0 + 13 * k + (d - 66 - 9 * k); }
  if (d < 209) { const int k = (d - 165) / 4; return CD_B0 + 13 * k + 9 + (d - 165 - 4 * k); }
  if (d < 221) return CD_EX0 + (d - 209);
  return CD_TD;
}

// dxs [VILO_MAX_PRIOR_DIM]: the prior's dx at the window's state, by block owner; inv_pmap [CD_N]: the prior row of a camera dimension, or -1.
// pmap: the window's prior_map (b.prior_map + 96 w), or a copy of it in LDS stored before the call. Two barriers: whatever the caller
// stored before the call is visible after it.
__device__ __forceinline__ void prior_view_init(const BatchDev &b, const WinMeta &wm, int w, const int *pmap, double *dxs, short *inv_pmap) {
  const int tid = threadIdx.x, pn = wm.prior_n;
  for (int e = tid; e < CD_N; e += GN_T) inv_pmap[e] = -1;
  if (pn > 0 && tid < wm.prior_nb) prior_dx_block(b, w, tid, b.x + (size_t)w * XSTRIDE, dxs);
  __syncthreads();
  if (tid < pn) inv_pmap[pmap[tid]] = (short)tid;
  __syncthreads();
}

// g += (J^T r)_cd and, if WANT_H, h += diag(J^T J)_cd of the active camera dimension cd, by one thread: its contributions in one fixed
// order — the window's visual Gram slots (chunks ascending, frame offsets ascending), the IMU Gram of interval f - 1 then of interval f,
// the prior's b0 + H dx and diag H — with plain adds in a register. Without WANT_H no diagonal entry is loaded and h is left alone.
template <bool WANT_H>
__device__ __forceinline__ void state_entry_gh(const BatchDev &b, const WinMeta &wm, int w, int cd, const short *inv_pmap, const double *dxs,
                                               double &g, double &h) {
  const int F = wm.n_frames, pn = wm.prior_n;
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
        if (WANT_H) h += gs[eh];
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
      if (f >= 1 && !b.imu_skip[w * 10 + f - 1]) {
        const double *gr = b.imu_gram + (size_t)(w * 10 + f - 1) * 780;
        g += gr[tri39(19 + ci, 38)];
        if (WANT_H) h += gr[tri39(19 + ci, 19 + ci)];
      }
      if (f + 1 < F && f < VILO_WINDOW_SIZE && !b.imu_skip[w * 10 + f]) {
        const double *gr = b.imu_gram + (size_t)(w * 10 + f) * 780;
        g += gr[tri39(ci, 38)];
        if (WANT_H) h += gr[tri39(ci, ci)];
      }
    }
  }
  // prior: J^T r = b0 + H dx, diag(J^T J) = diag H
  const int pi = inv_pmap[cd];
  if (pn > 0 && pi >= 0) {
    const double *Hp = b.prior_H + (size_t)w * 96 * 96;
    double s = b.prior_b0[(size_t)w * 96 + pi];
    for (int q = 0; q < pn; ++q) s += Hp[(size_t)q * pn + pi] * dxs[q];
    g += s;
    if (WANT_H) h += Hp[(size_t)pi * pn + pi];
  }
}

// Pm += the visual Gram slots (the 26-column view: pose s, pose s + t, ex0, ex1, td, r) of every chunk of the window's landmarks. One
// barrier per slot; the last one closes the function.
__device__ __forceinline__ void assemble_visual_pose_block(const BatchDev &b, const WinMeta &wm, double *Pm) {
  const int tid = threadIdx.x;
  for (int ch = 0; ch < wm.n_chunks; ++ch) {
    const ChunkMeta cm = b.chunk[wm.chunk_off + ch];
    for (int t = 0; t < cm.kmax; ++t) {
      const double *gs = b.gram + (size_t)(cm.gram_off + t) * VILO_GRAM;
      for (int e = tid; e < VILO_GRAM26; e += GN_T) {
        int a = 0, rem = e;
        while (rem >= 26 - a) { rem -= 26 - a; ++a; }
        const int bc = a + rem;
        if (bc == 25) continue;
        if (t == 0 && ((a >= 6 && a < 12) || (bc >= 6 && bc < 12))) continue;
        auto cdof = [&](int c) { return c < 6 ? 6 * cm.s + c : (c < 12 ? 6 * (cm.s + t) + (c - 6) : (c < 18 ? CD_EX0 + c - 12 : (c < 24 ? CD_EX1 + c - 18 : CD_TD))); };
        double sg;
        const double v = gs[gram26_index(a, bc, sg)];
        const int i = cdof(a), j = cdof(bc);
        Pm[i * GN_NP + j] += sg * v;
        if (i != j) Pm[j * GN_NP + i] += sg * v;
      }
      __syncthreads();
    }
  }
}

// Pm, Bd, Ao, BP += the IMU(-leg) Grams [pose_i 6 | B_i 13 | pose_j 6 | B_j 13 | r] (upper triangle) of the window's intervals. One barrier
// per interval.
__device__ __forceinline__ void assemble_imu_grams(const BatchDev &b, const WinMeta &wm, int w, double *Pm, double *Bd, double *Ao, double *BP) {
  const int tid = threadIdx.x;
  for (int k = 0; k + 1 < wm.n_frames && k < VILO_WINDOW_SIZE; ++k) {
    const int f = w * 10 + k;
    if (!b.imu_skip[f]) {
      const double *gr = b.imu_gram + (size_t)f * 780;
      for (int e = tid; e < 780; e += GN_T) {
        int a = 0, rem = e;
        while (rem >= 39 - a) { rem -= 39 - a; ++a; }
        const int bc = a + rem;   // (tri39(a, bc) == e)
        if (bc >= 38) continue;
        const double v = gr[e];
        auto map = [&](int c, bool &isP, int &fr) {   // P dimension or (frame, B dimension)
          if (c < 6) { isP = true; return 6 * k + c; }
          if (c < 19) { isP = false; fr = k; return c - 6; }
          if (c < 25) { isP = true; return 6 * (k + 1) + (c - 19); }
          isP = false; fr = k + 1; return c - 25;
        };
        bool pa, pb; int fa = 0, fb = 0;
        const int ia = map(a, pa, fa), ib = map(bc, pb, fb);
        if (pa && pb) { Pm[ia * GN_NP + ib] += v; if (ia != ib) Pm[ib * GN_NP + ia] += v; }
        else if (!pa && !pb) {
          if (fa == fb) { Bd[fa * 169 + ia * 13 + ib] += v; if (ia != ib) Bd[fa * 169 + ib * 13 + ia] += v; }
          else Ao[fb * 169 + ib * 13 + ia] += v;   // (a < bc: a in frame k, bc in frame k + 1)
        } else if (pa) BP[(fb * 13 + ib) * GN_NP + ia] += v;
        else BP[(fa * 13 + ia) * GN_NP + ib] += v;
      }
    }
    __syncthreads();
  }
}

// Pm, Bd, Ao, BP += H_prior on its camera dimensions (the whole n x n matrix: every target once). *bad (LDS) when the speed / bias part
// would not be block tridiagonal. One barrier at the end, if the window has a prior.
__device__ __forceinline__ void assemble_prior(const BatchDev &b, const WinMeta &wm, int w, double *Pm, double *Bd, double *Ao, double *BP, int *bad) {
  const int tid = threadIdx.x, pn = wm.prior_n;
  if (pn > 0) {
    const double *Hp = b.prior_H + (size_t)w * 96 * 96;
    const int *pmap = b.prior_map + (size_t)w * 96;
    for (int e = tid; e < pn * pn; e += GN_T) {
      const int ci = pmap[e / pn], cj = pmap[e % pn];
      const double v = Hp[e];
      if (ci < CD_B0 && cj < CD_B0) Pm[ci * GN_NP + cj] += v;
      else if (ci >= CD_B0 && cj >= CD_B0) {
        const int fi = (ci - CD_B0) / 13, di = (ci - CD_B0) % 13, fj = (cj - CD_B0) / 13, dj = (cj - CD_B0) % 13;
        if (fi == fj) Bd[fi * 169 + di * 13 + dj] += v;
        else if (fi == fj + 1) Ao[fi * 169 + di * 13 + dj] += v;
        else if (fj != fi + 1 && v != 0.0) *bad = 1;   // (no prior of the reference does this)
      } else if (ci >= CD_B0) BP[(ci - CD_B0) * GN_NP + cj] += v;
    }
    __syncthreads();
  }
}

// FRAME0 gauge, by one thread: Q = [e1 e2 u] (column-major: Q[3 m + i] = i-th entry of column m) from frame 0's quaternion q (qx qy qz qw),
// u = R0^T e_z. Frame 0's rotation is taken in this basis; the u direction and frame 0's position become constant dimensions.
__device__ __forceinline__ void gauge_basis(const double *q, double *Q) {
  const double qx = q[0], qy = q[1], qz = q[2], qw = q[3], nq = 1.0 / sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
  const double x = qx * nq, y = qy * nq, z = qz * nq, s = qw * nq;
  // u = third row of R0
  double u[3] = {2.0 * (x * z - s * y), 2.0 * (y * z + s * x), 1.0 - 2.0 * (x * x + y * y)};
  const double nu = 1.0 / sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  for (int i = 0; i < 3; ++i) u[i] *= nu;
  // e1 = normalise(u x a), a = the axis along which u is smallest; e2 = u x e1
  int m = 0;
  for (int i = 1; i < 3; ++i) if (fabs(u[i]) < fabs(u[m])) m = i;
  double a3[3] = {0.0, 0.0, 0.0}; a3[m] = 1.0;
  double e1[3] = {u[1] * a3[2] - u[2] * a3[1], u[2] * a3[0] - u[0] * a3[2], u[0] * a3[1] - u[1] * a3[0]};
  const double n1 = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
  for (int i = 0; i < 3; ++i) e1[i] *= n1;
  const double e2[3] = {u[1] * e1[2] - u[2] * e1[1], u[2] * e1[0] - u[0] * e1[2], u[0] * e1[1] - u[1] * e1[0]};
  for (int i = 0; i < 3; ++i) { Q[i] = e1[i]; Q[3 + i] = e2[i]; Q[6 + i] = u[i]; }
}

// H' = Q^T H Q on rows, then columns 3..5 of Pm and on columns 3..5 of BP. Q (LDS) must be visible (a barrier after gauge_basis); one
// barrier between the rows and the columns, one at the end.
__device__ __forceinline__ void gauge_rotate(double *Pm, double *BP, const double *Q) {
  const int tid = threadIdx.x;
  if (tid < GN_NP) {
    double r[3];
    for (int m = 0; m < 3; ++m) r[m] = Q[3 * m] * Pm[3 * GN_NP + tid] + Q[3 * m + 1] * Pm[4 * GN_NP + tid] + Q[3 * m + 2] * Pm[5 * GN_NP + tid];
    for (int m = 0; m < 3; ++m) Pm[(3 + m) * GN_NP + tid] = r[m];
  }
  __syncthreads();
  if (tid < GN_NP) {
    double r[3];
    for (int m = 0; m < 3; ++m) r[m] = Q[3 * m] * Pm[tid * GN_NP + 3] + Q[3 * m + 1] * Pm[tid * GN_NP + 4] + Q[3 * m + 2] * Pm[tid * GN_NP + 5];
    for (int m = 0; m < 3; ++m) Pm[tid * GN_NP + 3 + m] = r[m];
  }
  for (int rw = tid; rw < 143; rw += GN_T) {
    double *row = BP + (size_t)rw * GN_NP;
    double r[3];
    for (int m = 0; m < 3; ++m) r[m] = Q[3 * m] * row[3] + Q[3 * m + 1] * row[4] + Q[3 * m + 2] * row[5];
    for (int m = 0; m < 3; ++m) row[3 + m] = r[m];
  }
  __syncthreads();
}

// Jacobi scaling by dsc [CD_N] (0: a constant or absent dimension; its rows and columns become those of the identity, its coupling zero).
// No barrier: the caller places one before the scaled system is read.
__device__ __forceinline__ void scale_system(double *Pm, double *Bd, double *Ao, double *BP, const double *dsc) {
  const int tid = threadIdx.x;
  auto scaled = [&](double v, int ci, int cj) { const double di = dsc[ci], dj = dsc[cj]; return (di == 0.0 || dj == 0.0) ? (ci == cj ? 1.0 : 0.0) : v * di * dj; };
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Pm[e] = scaled(Pm[e], e / GN_NP, e % GN_NP);
  for (int e = tid; e < 11 * 169; e += GN_T) {
    const int k = e / 169, i = (e % 169) / 13, j = e % 13;
    Bd[e] = scaled(Bd[e], CD_B0 + 13 * k + i, CD_B0 + 13 * k + j);
    Ao[e] = k == 0 ? 0.0 : scaled(Ao[e], CD_B0 + 13 * k + i, CD_B0 + 13 * (k - 1) + j);
  }
  for (int e = tid; e < 143 * GN_NP; e += GN_T) {
    const double di = dsc[CD_B0 + e / GN_NP], dj = dsc[e % GN_NP];
    BP[e] = (di == 0.0 || dj == 0.0) ? 0.0 : BP[e] * di * dj;
  }
}

// in-place Cholesky of the 13 x 13 block ss in LDS (lower triangle; the upper one is not read afterwards). *bad (LDS) when a pivot <= thr.
// Barriers inside; the factor is visible on return.
__device__ __forceinline__ void chol13(double *ss, double thr, int *bad) {
  const int tid = threadIdx.x;
  for (int j = 0; j < 13; ++j) {
    if (tid == 0) {
      double p = ss[j * 13 + j];
      if (!(p > thr)) { *bad = 1; p = 1.0; }
      ss[j * 13 + j] = sqrt(p);
    }
    __syncthreads();
    if (tid > j && tid < 13) ss[tid * 13 + j] /= ss[j * 13 + j];
    __syncthreads();
    for (int e = tid; e < 169; e += GN_T) {
      const int r = e / 13, c = e % 13;
      if (c > j && r >= c) ss[e] -= ss[r * 13 + j] * ss[c * 13 + j];
    }
    __syncthreads();
  }
}

// D^2 / s^2 of a coordinate with Gauss-Newton diagonal h: s = 1 / (1 + sqrt(h)), D^2 = clamp(s^2 h, lo, hi)
__device__ __forceinline__ double step_dd(double h, double lo, double hi) {
  const double s = 1.0 / (1.0 + sqrt(h));
  return fmin(fmax(s * s * h, lo), hi) / (s * s);
}

// camera dimension of column c < 38 of interval k's IMU Gram [pose_k 6 | B_k 13 | pose_k+1 6 | B_k+1 13]
__device__ __forceinline__ int hv_imu_cd(int k, int c) {
  if (c < 6) return 6 * k + c;
  if (c < 19) return CD_B0 + 13 * k + (c - 6);
  if (c < 25) return 6 * (k + 1) + (c - 19);
  return CD_B0 + 13 * (k + 1) + (c - 25);
}

// one 16 x 16 tile of A X over nk k-steps of 4: A(i, k) for i = row0 + lr, X(k, column lr)
template <class FA, class FX>
__device__ __forceinline__ mfma_d4 hv_tile(int row0, int nk, int lr, int lk, FA A, FX X) {
  mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
  for (int ks = 0; ks < nk; ++ks) {
    const int kk = 4 * ks + lk;
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A(row0 + lr, kk), X(kk, lr), acc, 0, 0, 0);
  }
  return acc;
}
