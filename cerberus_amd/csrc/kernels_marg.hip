// Marginalisation half of Estimator::optimization() (estimator.cpp:1247-1455) and MarginalizationInfo
// (marginalization_factor.cpp:98-333) on gfx950: vilo_marginalize on host windows, vilo_batch_marginalize on a resident batch, and
// vilo_marginalize_batch inside vilo_optimize_windows (vilo_optimize.hip), where a window's new prior may go to a slot of a prior pool.
// The call is three steps: marg_plan (the block bookkeeping of marg_plan.hpp, no GPU), marg_run (upload, linearise, the kernels, the
// flags), marg_store (the priors into pool slots or host memory).
//
// The factors touching the dropped blocks are linearised by the same kernels the solver uses
// (k_visual_linearize / k_imu_linearize: residuals, Jacobians, Huber corrector), then one workgroup per window
//   * scatters J^T J / J^T r into A, b ordered [dropped | kept] (ThreadsConstructA, :150-181, without the 4 zero-
//     initialised thread-local copies),
//   * eigen-decomposes Amm by a parallel cyclic Jacobi method and forms the eps-thresholded pseudo-inverse (:281-286),
//   * forms the Schur complement A' = Arr - Arm Amm^+ Amr, b' = brr - Arm Amm^+ bmm (:289-295),
//   * eigen-decomposes A' and emits J0 = sqrt(S) V^T, r0 = sqrt(S^-1) V^T b' (:297-305).
// Address-keyed bookkeeping (addr_shift, estimator.cpp:1358-1370) is replaced by integer block ids.
#include <algorithm>
#include <type_traits>

#include "batch_call.hpp"
#include "cost_eval.hpp"
#include "marg_plan.hpp"
#include "solve_common.hpp"

using namespace vilo;


namespace {

#define MT 256

__device__ double blk_sum(double v, double *red) {
  const int t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (int s = MT / 2; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

// Parallel two-sided cyclic Jacobi: A (n x n symmetric, row-major, ld = n, global/L2) -> diag(A) = eigenvalues,
// V columns = eigenvectors. Round-robin pairing gives n/2 disjoint rotations per step; row phase then column phase.
__device__ void jacobi_eigh_dev(double *A, double *V, int n, double *cs /*LDS 2*(n/2+1)*/, int *pq /*LDS 2*(n/2+1)*/, double *red) {
  const int tid = threadIdx.x;
  for (int e = tid; e < n * n; e += MT) V[e] = (e / n == e % n) ? 1.0 : 0.0;
  __syncthreads();
  const int ne = (n + 1) & ~1, half = ne / 2;
  for (int sweep = 0; sweep < 60; ++sweep) {
    double off = 0.0, dg = 0.0;
    for (int e = tid; e < n * n; e += MT) {
      const int i = e / n, j = e % n;
      const double v = A[e];
      if (i == j) dg += v * v; else if (j > i) off += v * v;
    }
    off = blk_sum(off, red);
    dg = blk_sum(dg, red);
    if (off <= 1e-60 || off <= 1e-32 * dg) break;
    for (int step = 0; step < ne - 1; ++step) {
      if (tid < half) {
        // circle method: position tid plays position ne-1-tid; player at position k is (k == ne-1) ? ne-1 : (k + step) % (ne-1)
        const int ka = tid, kb = ne - 1 - tid;
        int p = (ka == ne - 1) ? ne - 1 : (ka + step) % (ne - 1);
        int q = (kb == ne - 1) ? ne - 1 : (kb + step) % (ne - 1);
        if (p > q) { const int t_ = p; p = q; q = t_; }
        double c = 1.0, s = 0.0;
        if (q < n) {
          const double apq = A[p * n + q];
          if (apq != 0.0) {
            const double app = A[p * n + p], aqq = A[q * n + q];
            const double tau = (aqq - app) / (2.0 * apq);
            const double t = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + t * t);
            s = t * c;
          }
        } else {
          q = -1;
        }
        pq[2 * tid] = p; pq[2 * tid + 1] = q;
        cs[2 * tid] = c; cs[2 * tid + 1] = s;
      }
      __syncthreads();
      // rows: A <- J^T A
      for (int e = tid; e < half * n; e += MT) {
        const int r = e / n, k = e % n;
        const int p = pq[2 * r], q = pq[2 * r + 1];
        if (q < 0) continue;
        const double c = cs[2 * r], s = cs[2 * r + 1];
        const double apk = A[p * n + k], aqk = A[q * n + k];
        A[p * n + k] = c * apk - s * aqk;
        A[q * n + k] = s * apk + c * aqk;
      }
      __syncthreads();
      // columns: A <- A J, V <- V J
      for (int e = tid; e < half * n; e += MT) {
        const int r = e / n, k = e % n;
        const int p = pq[2 * r], q = pq[2 * r + 1];
        if (q < 0) continue;
        const double c = cs[2 * r], s = cs[2 * r + 1];
        const double akp = A[k * n + p], akq = A[k * n + q];
        A[k * n + p] = c * akp - s * akq;
        A[k * n + q] = s * akp + c * akq;
        const double vkp = V[k * n + p], vkq = V[k * n + q];
        V[k * n + p] = c * vkp - s * vkq;
        V[k * n + q] = s * vkp + c * vkq;
      }
      __syncthreads();
    }
  }
  __syncthreads();
}

// scratch layout per window (doubles): A (T*T) | b (T) | Amm (m*m) | Vm (m*m) | Ainv (m*m) | tmp (n*m) | Ar (n*n) | V2 (n*n) | br (n)
__global__ void __launch_bounds__(MT) k_marginalize(BatchDev bd, const MargWin *mw, const int *drop_lm /*[W][maxL0] device-order local idx*/,
                                                    int max_l0, double *scratch, double *J0_out, double *r0_out, int *status) {
  __shared__ double red[MT];
  __shared__ double cs[2 * 600];
  __shared__ int pq[2 * 600];
  __shared__ double dx[VILO_MAX_PRIOR_DIM];
  const int win = blockIdx.x, tid = threadIdx.x;
  const MargWin &M = mw[win];
  const WinMeta wm = bd.win[win];
  const int m = M.m, n = M.n, T = m + n;
  if (m == 0 || n == 0 || !M.general) return;
  double *A = scratch + M.scratch_off, *bv = A + (size_t)T * T, *Amm = bv + T, *Vm = Amm + (size_t)m * m, *Ainv = Vm + (size_t)m * m;
  double *tmp = Ainv + (size_t)m * m, *Ar = tmp + (size_t)n * m, *V2 = Ar + (size_t)n * n, *br = V2 + (size_t)n * n;
  const double *x = bd.x + (size_t)win * XSTRIDE;
  for (size_t e = tid; e < (size_t)T * T + T; e += MT) A[e] = 0.0;
  __syncthreads();
  auto add = [&](int ci, int cj, double v) {   // camera dims -> A
    const int i = M.cdmap[ci], j = M.cdmap[cj];
    if (i >= 0 && j >= 0) A[(size_t)i * T + j] += v;
  };
  // ---- prior factor: J^T J = H_prior, J^T r = b0 + H_prior dx ----
  if (M.prior_n > 0) {
    const int pn = M.prior_n;
    const double *Hp = bd.prior_H + (size_t)win * 96 * 96, *b0 = bd.prior_b0 + (size_t)win * 96;
    const int *pmap = bd.prior_map + (size_t)win * 96;
    if (tid < wm.prior_nb) prior_dx_block(bd, win, tid, x, dx);
    __syncthreads();
    for (int e = tid; e < pn * pn; e += MT) add(pmap[e / pn], pmap[e % pn], Hp[e]);
    for (int i = tid; i < pn; i += MT) {
      double s = b0[i];
      for (int q = 0; q < pn; ++q) s += Hp[(size_t)q * pn + i] * dx[q];
      const int t = M.cdmap[pmap[i]];
      if (t >= 0) bv[t] += s;
    }
    __syncthreads();
  }
  if (M.mode == 0) {
    // ---- IMULegFactor(0, 1) ----
    if (M.has_imu) {
      const double *lin = bd.imu_lin + (size_t)win * 10 * 31 * 39;
      for (int e = tid; e < 39 * 39; e += MT) {
        const int a = e / 39, c = e % 39;
        if (a == 38) continue;
        double s = 0.0;
        for (int i = 0; i < 31; ++i) s += lin[i * 39 + a] * lin[i * 39 + c];
        auto cdof = [](int cc) { return cc < 6 ? cc : (cc < 19 ? CD_B0 + (cc - 6) : (cc < 25 ? 6 + (cc - 19) : CD_B0 + 13 + (cc - 25))); };
        if (c == 38) { const int t = M.cdmap[cdof(a)]; if (t >= 0) bv[t] += s; }
        else add(cdof(a), cdof(c), s);
      }
      __syncthreads();
    }
    // ---- visual factors of the landmarks that start in frame 0: camera-side Gram slots of the s = 0 chunks ----
    for (int ch = 0; ch < wm.n_chunks; ++ch) {
      const ChunkMeta cm = bd.chunk[wm.chunk_off + ch];
      if (cm.s != 0) continue;
      for (int t = 0; t < cm.kmax; ++t) {
        const double *gs = bd.gram + (size_t)(cm.gram_off + t) * VILO_GRAM;
        for (int e = tid; e < VILO_GRAM26; e += MT) {   // the 26-column view of the slot
          int a = 0, rem = e;
          while (rem >= 26 - a) { rem -= 26 - a; ++a; }
          const int bc = a + rem;
          if (t == 0 && ((a >= 6 && a < 12) || (bc >= 6 && bc < 12))) continue;
          auto cdof = [&](int c) { return c < 6 ? c : (c < 12 ? 6 * t + (c - 6) : (c < 18 ? CD_EX0 + c - 12 : (c < 24 ? CD_EX1 + c - 18 : CD_TD))); };
          double sg;
          const int ge = gram26_index(a, bc, sg);
          const double v = sg * gs[ge];
          if (bc == 25) { if (a < 25) { const int q = M.cdmap[cdof(a)]; if (q >= 0) bv[q] += v; } }
          else {
            add(cdof(a), cdof(bc), v);
            if (cdof(a) != cdof(bc)) add(cdof(bc), cdof(a), v);
          }
        }
        __syncthreads();
      }
    }
    // landmark (inverse depth) rows / columns
    const double *wl = bd.lm_w + 80 * (size_t)wm.lm_off;
    for (int e = tid; e < M.n_drop_lm * 80; e += MT) {
      const int li = e / 80, a = e % 80;
      const int l = drop_lm[(size_t)win * max_l0 + li];
      const int row = M.m - M.n_drop_lm + li;   // landmarks follow the dropped frame-0 dims (19 with leg biases, 15 without)
      if (a == 79) {
        A[(size_t)row * T + row] += bd.lm_E[wm.lm_off + l];
        bv[row] += bd.lm_gbuf[0][wm.lm_off + l];
      } else {
        const int t = M.cdmap[a];
        const double v = wl[(size_t)a * wm.L + l];
        if (t >= 0) { A[(size_t)row * T + t] += v; A[(size_t)t * T + row] += v; }
      }
    }
    __syncthreads();
  }
  // ---- Amm = 1/2 (Amm + Amm^T), eigen, pseudo-inverse (eps = 1e-8) ----
  const double eps = 1e-8;
  for (int e = tid; e < m * m; e += MT) {
    const int i = e / m, j = e % m;
    Amm[e] = 0.5 * (A[(size_t)i * T + j] + A[(size_t)j * T + i]);
  }
  __syncthreads();
  jacobi_eigh_dev(Amm, Vm, m, cs, pq, red);
  for (int e = tid; e < m * m; e += MT) {
    const int i = e / m, j = e % m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) {
      const double w = Amm[(size_t)k * m + k];
      if (w > eps) s += Vm[(size_t)i * m + k] * (1.0 / w) * Vm[(size_t)j * m + k];
    }
    Ainv[e] = s;
  }
  __syncthreads();
  // tmp = Arm Amm^+ ; A' = Arr - tmp Amr ; b' = brr - tmp bmm
  for (int e = tid; e < n * m; e += MT) {
    const int i = e / m, j = e % m;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += A[(size_t)(m + i) * T + k] * Ainv[(size_t)k * m + j];
    tmp[e] = s;
  }
  __syncthreads();
  for (int e = tid; e < n * n; e += MT) {
    const int i = e / n, j = e % n;
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += tmp[(size_t)i * m + k] * A[(size_t)k * T + m + j];
    Ar[e] = A[(size_t)(m + i) * T + m + j] - s;
  }
  for (int i = tid; i < n; i += MT) {
    double s = 0.0;
    for (int k = 0; k < m; ++k) s += tmp[(size_t)i * m + k] * bv[k];
    br[i] = bv[m + i] - s;
  }
  __syncthreads();
  // SelfAdjointEigenSolver reads the lower triangle: symmetrise from it
  for (int e = tid; e < n * n; e += MT) {
    const int i = e / n, j = e % n;
    if (j > i) Ar[e] = Ar[(size_t)j * n + i];
  }
  __syncthreads();
  // keep A' for the caller's invariants before it is diagonalised: stored after br
  double *Akeep = br + n;
  for (int e = tid; e < n * n; e += MT) Akeep[e] = Ar[e];
  __syncthreads();
  jacobi_eigh_dev(Ar, V2, n, cs, pq, red);
  double *J0 = J0_out + (size_t)win * VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM, *r0 = r0_out + (size_t)win * VILO_MAX_PRIOR_DIM;
  for (int e = tid; e < n * n; e += MT) {
    const int i = e / n, j = e % n;
    const double S = Ar[(size_t)i * n + i];
    J0[e] = (S > eps) ? sqrt(S) * V2[(size_t)j * n + i] : 0.0;
  }
  for (int i = tid; i < n; i += MT) {
    const double S = Ar[(size_t)i * n + i];
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += V2[(size_t)j * n + i] * br[j];
    r0[i] = (S > eps) ? sqrt(1.0 / S) * s : 0.0;
    if (!isfinite(r0[i])) status[win] = 1;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// LDS-resident marginalisation (the path every well-conditioned window takes).
//
// MarginalizationInfo::marginalize inverts Amm through an eigen-decomposition with eigenvalues <= eps = 1e-8 dropped
// (marginalization_factor.cpp:281-286). When every eigenvalue of Amm exceeds eps that pseudo-inverse IS the inverse, and the
// Schur complement can be formed by elimination in the order the block structure suggests: the dropped landmarks first (their
// block of Amm is diagonal: an inverse depth only couples to camera-side blocks), then the <= 19 dense dims of frame 0 by a
// Cholesky factorisation. The kernel certifies "lambda_min(Amm) > eps" by factorising Amm - eps I the same way (all pivots
// positive) and hands the window to k_marginalize (global-memory Jacobi on the full Amm) when the certificate fails.
// The second decomposition (A' -> J0 = sqrt(S) V^T, marginalization_factor.cpp:297-305) needs a rank decision (a first prior carries
// the unobservable gauge directions) and the products sqrt(S) V^T, S^-1/2 V^T b, not V itself: prior_factor_lds below.
#define MGT 1024
constexpr int MG_NMAX = VILO_MAX_PRIOR_DIM;       // 96
constexpr int MG_LD = MG_NMAX + 1;                // odd leading dimension: column walks spread over the LDS banks
constexpr int MG_TMAX = 19 + MG_NMAX;             // dense dropped dims + kept dims
constexpr int MG_TILE = 32;                       // landmarks per elimination tile
constexpr int MG_R0 = 2 * MG_NMAX * MG_LD;        // 18624 doubles: A1 (TMAX^2 = 13225) + tile (TMAX * 32), later A' | V
constexpr int MG_TILE_OFF = 13312;
constexpr int MG_SMALL = MG_TMAX + 3 * MG_TILE + 19 * 19 + 2 * 48 + 19 + MG_NMAX + 8;
constexpr int MG_LDS_DOUBLES = MG_R0 + MG_SMALL;
static_assert(MG_TILE_OFF >= MG_TMAX * MG_TMAX && MG_TILE_OFF + MG_TMAX * MG_TILE <= MG_R0, "LDS plan");
static_assert(MG_LDS_DOUBLES * 8 + 2 * 80 * 4 + 96 * 8 + 2 * 96 * 8 + 64 <= 160 * 1024, "LDS budget");   // dynamic + act_a / act_t, dx, dgb, flags

// in-place Cholesky of the leading d x d block (lower triangle) of M; all threads call. *fail is set when a pivot is not positive.
__device__ void chol_lds(double *M, int ld, int d, int *fail) {
  const int tid = threadIdx.x;
  for (int k = 0; k < d; ++k) {
    if (tid == 0) {
      const double p = M[k * ld + k];
      if (!(p > 0.0)) { *fail = 1; M[k * ld + k] = 1.0; } else M[k * ld + k] = sqrt(p);
    }
    __syncthreads();
    if (tid > k && tid < d) M[tid * ld + k] /= M[k * ld + k];
    __syncthreads();
    for (int e = tid; e < d * d; e += MGT) {
      const int i = e / d, j = e % d;
      if (j > k && i >= j) M[i * ld + j] -= M[i * ld + k] * M[j * ld + k];
    }
    __syncthreads();
  }
}

// A' -> J0, r0 (marginalization_factor.cpp:297-305: J0 = sqrt(S) V^T, r0 = S^-1/2 V^T b over the eigenpairs with S > eps) without forming V.
//
// With A' = X X^T, rotating the columns of X from the right until they are mutually orthogonal (one-sided Jacobi, Hestenes) leaves
// X = V sqrt(S): the columns ARE the rows of J0, their squared norms the eigenvalues, r0_i = x_i^T b / S_i, and X X^T = A' holds after
// every rotation, so J0^T J0 = A' to rounding whatever the state of convergence (which only decides the eps threshold and r0).
//   1. X from a diagonally pivoted Cholesky without row exchanges: step k takes the largest remaining diagonal entry j, column
//      k of X = A[:, j] / sqrt(A[j][j]) over the rows not yet taken, A -= x_k x_k^T. It stops at the first pivot <= 0: a
//      semi-definite A' (the 4 gauge directions of a first prior) gives r < n columns. Jacobi then works on X^T X = L^T L, one
//      step of the LR iteration past A'.
//   2. Pair i of a step = the two columns lane i holds in registers (its "top" and "bottom"), 12 rows of them per wave (8 of the 16
//      waves). A step: every wave leaves the three partial dot products of its rows in LDS, wave 0 sums them and computes the rotation
//      of every pair, every wave rotates its rows and makes the round-robin tournament's move inside the registers (tops one lane up,
//      bottoms one lane down: v_mov_b32_dpp wave_shr:1 / wave_shl:1). The matrix never touches LDS inside the sweeps.
//   3. Sweeps end when the largest |cos| a sweep met is <= 1e-7 (quadratic convergence: the sweep itself took it to 1e-14).
// 1 / sqrt(x) to double rounding: v_rsq_f64 (about 2^-23) and two Newton steps
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
  y = y * (1.5 - hx * y * y);
  y = y * (1.5 - hx * y * y);
  return y;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_max_step(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xF, false);
  return fmax(v, __hiloint2double(hi, lo));
}
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double old, double src) {
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}
// max over the wave of non-negative values (0.0 is the identity the DPP steps shift in), the same in every lane: prefix maxima within
// each row of 16 lanes (row_shr 1, 2, 4, 8), row_bcast15 / row_bcast31 across rows, lane 63 holds the result
__device__ __forceinline__ double wave_max_nonneg(double v) {
  v = dpp_max_step<0x111, 0xF>(v);
  v = dpp_max_step<0x112, 0xF>(v);
  v = dpp_max_step<0x114, 0xF>(v);
  v = dpp_max_step<0x118, 0xF>(v);
  v = dpp_max_step<0x142, 0xA>(v);
  v = dpp_max_step<0x143, 0xC>(v);
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}

// The sweeps of prior_factor_lds for JR row slots per wave (rows wv + JW * i, i < JR; JW * JR >= n): see the comment above it.
constexpr int JW = 8;   // waves that hold rows
template <int JR>
__device__ __forceinline__ void jacobi_sweeps(double *P, double *part /* [3][JW][48] */, double *cs, int *conv_s, int ne) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, h = ne >> 1;
  const bool act = lane < h && wv < JW;
  const int lc = min(lane, 47);
  double t[JR], b[JR];   // this wave's JR rows of the two columns of pair `lane`
#pragma unroll
  for (int i = 0; i < JR; ++i) {
    const double tv = P[lc * MG_LD + wv % JW + JW * i], bv = P[min(h + lc, MG_NMAX - 1) * MG_LD + wv % JW + JW * i];
    t[i] = act ? tv : 0.0;
    b[i] = act ? bv : 0.0;
  }
  __syncthreads();
  const bool first = lane == 0, last = lane == h - 1;
  double na = 0.0, nb = 0.0;   // wave 0: squared norms of the two columns of pair `lane`
  for (int sweep = 0; sweep < 30; ++sweep) {
    double mx = 0.0;   // largest cos^2 this sweep rotated away (wave 0)
    // squared column norms from the data once per sweep; inside the sweep they follow the rotations in closed form
    // (|x_p'|^2 = c^2 a - 2 c s g + s^2 b, |x_q'|^2 = s^2 a + 2 c s g + c^2 b) and travel with their columns
    if (wv < JW) {
      double a_ = 0.0, b_ = 0.0;
#pragma unroll
      for (int i = 0; i < JR; ++i) { a_ += t[i] * t[i]; b_ += b[i] * b[i]; }
      if (act) { part[wv * 48 + lane] = a_; part[(JW + wv) * 48 + lane] = b_; }
    }
    __syncthreads();
    if (wv == 0) {
      na = 0.0; nb = 0.0;
#pragma unroll
      for (int w = 0; w < JW; ++w) { na += part[w * 48 + lc]; nb += part[(JW + w) * 48 + lc]; }
    }
    for (int step = 0; step < ne - 1; ++step) {
      if (wv < JW) {
        double g_ = 0.0;
#pragma unroll
        for (int i = 0; i < JR; ++i) g_ += t[i] * b[i];
        if (act) part[(2 * JW + wv) * 48 + lane] = g_;
      }
      __syncthreads();
      if (wv == 0) {   // all 64 lanes: the norms move by DPP like the columns; lanes >= h carry values nobody reads
        double sg = 0.0;
#pragma unroll
        for (int w = 0; w < JW; ++w) sg += part[(2 * JW + w) * 48 + lc];
        // tan 2 theta = 2 sg / (nb - na), |theta| <= pi / 4: cos 2 theta = |zeta| / hyp, c = sqrt((1 + cos 2 theta) / 2), s = sin 2 theta / (2 c)
        double c = 1.0, sn = 0.0;
        const double ab = na * nb, g2 = sg * sg;
        const double zeta = nb - na, gam = 2.0 * sg, hyp2 = zeta * zeta + gam * gam;
        if (act && g2 > 1e-28 * ab && hyp2 > 1e-290) {
          mx = fmax(mx, g2 * __builtin_amdgcn_rcp(ab));
          const double rh = rsqrt_nr(hyp2);
          const double c2 = fabs(zeta) * rh, s2 = (zeta >= 0.0 ? gam : -gam) * rh;
          const double hc = 0.5 + 0.5 * c2, rc = rsqrt_nr(hc);
          c = hc * rc;
          sn = 0.5 * s2 * rc;
        }
        if (act) { cs[2 * lane] = c; cs[2 * lane + 1] = sn; }
        const double cc = c * c, ss = sn * sn, x2 = 2.0 * c * sn * sg;
        const double an = fmax(cc * na - x2 + ss * nb, 0.0), bn = fmax(ss * na + x2 + cc * nb, 0.0);
        na = dpp_mov<0x138>(an, first ? bn : an);
        const double bd = dpp_mov<0x130>(bn, bn);
        nb = last ? an : bd;
      }
      __syncthreads();
      if (wv < JW) {
        // rotate, then the round-robin move inside the registers: tops go one lane up (lane 0 keeps its own, lane 1 takes lane 0's
        // bottom), bottoms one lane down (lane h - 1 takes its own top). All 64 lanes run this: a DPP move reads its neighbour's register.
        const double c = cs[2 * lc], sn = cs[2 * lc + 1];
#pragma unroll
        for (int i = 0; i < JR; ++i) {
          const double tn = c * t[i] - sn * b[i], bn = sn * t[i] + c * b[i];
          const double send = first ? bn : tn;
          const double bd = dpp_mov<0x130>(bn, bn);     // wave_shl:1
          b[i] = last ? tn : bd;
          t[i] = dpp_mov<0x138>(tn, send);              // wave_shr:1 (tn's last use: the move can land in its register)
        }
      }
    }
    if (wv == 0) {
      mx = wave_max_nonneg(mx);
      if (lane == 0) *conv_s = (mx <= 1e-14) ? 1 : 0;
    }
    __syncthreads();
    if (*conv_s) break;
  }
  if (act) {
#pragma unroll
    for (int i = 0; i < JR; ++i) { P[lane * MG_LD + wv + JW * i] = t[i]; P[(h + lane) * MG_LD + wv + JW * i] = b[i]; }
  }
}

// factor_form (vilo_set_prior_form(ctx, VILO_PRIOR_FACTOR): callers that never look at J0 itself — a resident prior pool): the prior is
// only ever used through J0^T J0, J0^T r0 and |r0|^2, which any X with X X^T = A' gives alike with J0 = X^T, r0 = X^-1 b — the reference's
// sqrt(S) V^T is Q X^T for an orthogonal Q. What the eigen form adds is the threshold: eigenvalues <= eps are dropped
// (marginalization_factor.cpp:297-305). So the pivoted Cholesky factor is taken as it stands IF it has full rank AND lambda_min(A') > eps is
// certain: lambda_min = 1 / |X^-1|_2^2 >= 1 / |X^-1|_F^2, and X^-1 comes out of the same forward substitutions that give r0 (n unit
// right-hand sides beside b, 8 lanes per column; ~30 k cycles instead of the sweeps' 1.5 M). Anything else goes on to the sweeps.
__device__ void prior_factor_lds(double *Ar /* n x n, ld MG_LD, bitwise symmetric, destroyed */, double *P /* MG_NMAX x MG_LD */, const double *br, int n, double eps,
                                 double *cs /* LDS [96] */, double *J0, double *r0, int *status_w, long long *clk_w /* [8] or null */, bool factor_form) {
  __shared__ int bad, conv, fast_ok;
  __shared__ int piv[MG_NMAX];
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int ty = tid >> 5, tx = tid & 31;
  for (int e = tid; e < MG_NMAX * MG_LD; e += MGT) P[e] = 0.0;
  if (tid == 0) bad = 0;
  __syncthreads();
  {
    bool nf = false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)
        if (ty + 32 * a < n && tx + 32 * b < n) nf |= !isfinite(Ar[(ty + 32 * a) * MG_LD + tx + 32 * b]);
    if (tid < n) nf |= !isfinite(br[tid]);
    if (nf) bad = 1;
  }
  // ---- pivoted Cholesky, left-looking, one barrier per step. A' stays as it is; the running diagonal lives in LDS (dg), the finished
  //      columns of X in LDS (P, for the pivot row) and in registers: thread (i, q) = (tid / 8, tid % 8) keeps X[i][q + 8 m], m < 12.
  //      Step k: every wave finds the pivot j for itself (diagonal entry with its index in the low 7 mantissa bits, so one DPP max decides
  //      value and index; ties go to the smaller index; taken rows carry 0), then x_i = (A[i][j] - sum_k' X[i][k'] X[j][k']) / sqrt(d_j):
  //      12 products per thread (columns >= k of P are still zero, so the sum needs no bound) and a sum over the 8 lanes of the row. ----
  int r = 0;
  {
    __shared__ double dgb[2][MG_NMAX];   // the diagonal, double-buffered: step k reads [k & 1] while the finished rows write [(k + 1) & 1]
    __shared__ double dinv0[MG_NMAX];   // 1 / (the diagonal A' started with): what a remaining diagonal entry is measured against (factor form)
    if (tid < MG_NMAX) {
      const double d_ = (tid < n) ? Ar[tid * (MG_LD + 1)] : 0.0;
      dgb[0][tid] = d_;
      dinv0[tid] = (d_ > 0.0) ? 1.0 / d_ : 0.0;
    }
    __syncthreads();
    const int ri = tid >> 3, rq = tid & 7, ric = min(ri, MG_NMAX - 1);
    bool taken = ri >= n;
    double xs[12];
#pragma unroll
    for (int m = 0; m < 12; ++m) xs[m] = 0.0;
    const int l1 = min(lane + 64, MG_NMAX - 1);
    // columns in blocks of 8 with the block index a compile-time constant: the sum runs over the blocks that exist, and the new entry
    // goes into a register the code names
    bool done = false;
    auto block = [&](auto mbc) {
      constexpr int mb = decltype(mbc)::value;
      if (done || 8 * mb >= n) return;
      for (int k = 8 * mb; k < min(8 * mb + 8, n); ++k) {
        const double *dg = dgb[k & 1];
        const double d0 = dg[lane], d1 = (lane + 64 < MG_NMAX) ? dg[l1] : 0.0;
        double best = 0.0;
        if (d0 > 0.0) best = __hiloint2double(__double2hiint(d0), (__double2loint(d0) & ~127) | (127 - lane));
        if (d1 > 0.0) best = fmax(best, __hiloint2double(__double2hiint(d1), (__double2loint(d1) & ~127) | (63 - lane)));
        best = wave_max_nonneg(best);
        if (!(best > 0.0)) { done = true; break; }
        // factor form: what is left of A' is positive semi-definite with trace <= (n - k) * (largest diagonal entry); once that is <= eps
        // every eigenvalue of the remainder is, and the eigen form would drop them too (a sequence's prior never fixes the four gauge
        // directions: their pivots come out as +- 1e-9 noise, and a factor that carried them on could not be certified below)
        if (factor_form) {
          if (best * (double)(n - k) <= eps) { done = true; break; }
          // ... or when every remaining diagonal entry is rounding noise of the entry it started as (<= 1e-12 of it: n u times the growth
          // of the elimination) — with information up to 1e15 in A' the gauge pivots come out as +- 1e-2, far above eps, and an eigen
          // decomposition keeps or drops such a direction by the sign its noise happens to have
          const double rel = wave_max_nonneg(fmax(d0 * dinv0[lane], d1 * ((lane + 64 < MG_NMAX) ? dinv0[l1] : 0.0)));
          if (rel <= 1e-12) { done = true; break; }
        }
        const int j = 127 - (__double2loint(best) & 127);
        const double pv = dg[j], aij = Ar[ric * MG_LD + j];
        double acc = 0.0;
#pragma unroll
        for (int m = 0; m <= mb; ++m) acc += xs[m] * P[(rq + 8 * m) * MG_LD + j];   // columns >= k of P, if a faster wave wrote them, meet xs = 0
        acc += dpp_mov<0xB1>(0.0, acc);    // quad_perm [1, 0, 3, 2]
        acc += dpp_mov<0x4E>(0.0, acc);    // quad_perm [2, 3, 0, 1]
        acc += dpp_mov<0x141>(0.0, acc);   // row_half_mirror: the other quad of the 8 lanes
        const double rs = rsqrt_nr(pv);
        const double x = taken ? 0.0 : (ri == j ? pv * rs : (aij - acc) * rs);
        taken |= (ri == j);
        xs[mb] = (rq == (k & 7)) ? x : xs[mb];
        if (rq == 0 && ri < MG_NMAX) {
          P[k * MG_LD + ri] = x;
          dgb[(k + 1) & 1][ri] = taken ? 0.0 : dg[ri] - x * x;
        }
        if (tid == 0) piv[k] = j;
        __syncthreads();
        ++r;
      }
    };
    block(std::integral_constant<int, 0>{}); block(std::integral_constant<int, 1>{}); block(std::integral_constant<int, 2>{});
    block(std::integral_constant<int, 3>{}); block(std::integral_constant<int, 4>{}); block(std::integral_constant<int, 5>{});
    block(std::integral_constant<int, 6>{}); block(std::integral_constant<int, 7>{}); block(std::integral_constant<int, 8>{});
    block(std::integral_constant<int, 9>{}); block(std::integral_constant<int, 10>{}); block(std::integral_constant<int, 11>{});
  }
  __syncthreads();
  if (clk_w && tid == 0) clk_w[7] = (long long)__builtin_readcyclecounter();
  if (factor_form && r >= 1) {
    // X (n x r, r <= n: a semi-definite A' — the four gauge directions no prior of a sequence ever fixes — stops the factorisation at the
    // first pivot <= 0, and what is left of A' then is rounding noise the eigen form drops as well). Its pivot rows form a lower triangle
    // X_p in pivot order; sigma_min(X) >= sigma_min(X_p) >= 1 / |X_p^-1|_F. X_p y = v by forward substitution: step k fixes y[k] from row
    // piv[k]. Column c < r: v = e_c (a column of X_p^-1); column r: v = b on the pivot rows (b lies in the range of A' up to rounding, so
    // J0^T r0 = X X_p^-1 b_p reproduces it). Thread (c, q) = (tid / 8, tid % 8) sums the products k' = q mod 8; Y[k][c] in the spent A'.
    double *Y = Ar;
    const int c = tid >> 3, q = tid & 7, cc = min(c, r);
    double ssq = 0.0;
    for (int k = 0; k < r; ++k) {
      const int j = piv[k];
      double acc = 0.0;
      for (int kk = q; kk < k; kk += 8) acc += P[kk * MG_LD + j] * Y[kk * MG_LD + cc];
      acc += dpp_mov<0xB1>(0.0, acc);
      acc += dpp_mov<0x4E>(0.0, acc);
      acc += dpp_mov<0x141>(0.0, acc);
      if (q == 0 && c <= r) {
        const double rhs = (c < r) ? (c == k ? 1.0 : 0.0) : br[j];
        const double y = (rhs - acc) / P[k * MG_LD + j];
        Y[k * MG_LD + c] = y;
        if (c < r) ssq += y * y;
      }
      lds_fence();   // (the column's next step reads what lane q == 0 of these 8 lanes just wrote: same wave, LDS operations in order)
    }
    if (tid == 0) fast_ok = 0;
    if (tid < MG_NMAX) cs[tid] = 0.0;
    __syncthreads();
    if (q == 0 && c < r) cs[c] = ssq;
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      for (int i = 0; i < r; ++i) tot += cs[i];
      fast_ok = (isfinite(tot) && tot * eps < 1.0) ? 1 : 0;   // 1 / |X_p^-1|_F^2 > eps: no eigenvalue of X X^T in (0, eps]
    }
    __syncthreads();
    if (fast_ok) {
      if (tid < n) {
        const double rv = (tid < r) ? Y[tid * MG_LD + r] : 0.0;
        r0[tid] = rv;
        if (!isfinite(rv) || bad) *status_w = 1;
      }
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const int i = ty + 32 * a;
        if (i >= n) continue;
        for (int j = tx; j < n; j += 32) J0[i * n + j] = (i < r) ? P[i * MG_LD + j] : 0.0;
      }
      if (clk_w && tid == 0) clk_w[5] = (long long)__builtin_readcyclecounter();
      return;
    }
    __syncthreads();
  }
  const int ne = max(4, (r + 1) & ~1), h = ne >> 1;   // zero columns fill up; at least two pairs, so the move below has no special case
  static_assert(JW * 12 >= MG_NMAX && JW <= MGT / 64, "row split of the Jacobi sweeps");
  double *part = Ar;   // [3][JW][48] partial dot products; A' is spent
  if (n <= JW * 10) jacobi_sweeps<10>(P, part, cs, &conv, ne);
  else if (n <= JW * 11) jacobi_sweeps<11>(P, part, cs, &conv, ne);
  else jacobi_sweeps<12>(P, part, cs, &conv, ne);
  __syncthreads();
  if (clk_w && tid == 0) clk_w[5] = (long long)__builtin_readcyclecounter();
  // eigenvalue of position i = |x_i|^2; after whole sweeps every column is back at the position it started from, any order of the rows of J0 is as good
  if (tid < MG_NMAX) {
    double S = 0.0, xb = 0.0;
    if (tid < ne)
      for (int row = 0; row < n; ++row) { const double v = P[tid * MG_LD + row]; S += v * v; xb += v * br[row]; }
    cs[tid] = S;
    if (tid < n) {
      const double rv = (S > eps) ? xb / S : 0.0;
      r0[tid] = rv;
      if (!isfinite(rv) || bad) *status_w = 1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int i = ty + 32 * a;
    if (i >= n) continue;
    const bool keep = cs[i] > eps;
    for (int j = tx; j < n; j += 32) J0[i * n + j] = keep ? P[i * MG_LD + j] : 0.0;
  }
}

__global__ void __launch_bounds__(MGT) k_marginalize_lds(BatchDev bd, const MargWin *mw, const int *drop_lm, int max_l0, double *J0_out,
                                                         double *r0_out, int *status, int *need_general, long long *clk /* [W][8] or null */, int factor_form) {
  extern __shared__ double ml[];
  double *A1 = ml, *tile = ml + MG_TILE_OFF;
  double *b1 = ml + MG_R0, *dinv = b1 + MG_TMAX, *deps = dinv + MG_TILE, *gl = deps + MG_TILE, *Ce = gl + MG_TILE, *cs = Ce + 19 * 19;
  double *yb = cs + 2 * 48, *br = yb + 19;
  __shared__ int act_a[80], act_t[80];
  __shared__ int n_act, fail;
  __shared__ double dx[VILO_MAX_PRIOR_DIM];
  const int win = blockIdx.x, tid = threadIdx.x;
  const MargWin &M = mw[win];
  const WinMeta wm = bd.win[win];
  const int m = M.m, n = M.n, L0 = M.n_drop_lm, md = m - L0, T = md + n;
  if (m == 0 || n == 0) return;
  if (T > MG_TMAX || n > MG_NMAX || md > 19) { if (tid == 0) need_general[win] = 1; return; }
  const double eps = 1e-8;
  const double *x = bd.x + (size_t)win * XSTRIDE;
  auto stamp = [&](int i) { if (clk && tid == 0) clk[win * 8 + i] = (long long)__builtin_readcyclecounter(); };
  stamp(0);
  // index of a camera dim in [dense dropped | kept], -1 if absent
  auto loc = [&](int ci) { const int i = M.cdmap[ci]; return i < 0 ? -1 : (i < md ? i : i - L0); };
  for (int e = tid; e < T * T; e += MGT) A1[e] = 0.0;
  for (int e = tid; e < T; e += MGT) b1[e] = 0.0;
  if (tid == 0) { n_act = 0; fail = 0; }
  __syncthreads();
  auto add = [&](int ci, int cj, double v) {
    const int i = loc(ci), j = loc(cj);
    if (i >= 0 && j >= 0) A1[i * T + j] += v;
  };
  // ---- prior factor (marginalization_factor.cpp:347-395 evaluated at the current state): J^T J = H, J^T r = b0 + H dx ----
  if (M.prior_n > 0) {
    const int pn = M.prior_n;
    const double *Hp = bd.prior_H + (size_t)win * 96 * 96, *b0 = bd.prior_b0 + (size_t)win * 96;
    const int *pmap = bd.prior_map + (size_t)win * 96;
    if (tid < wm.prior_nb) prior_dx_block(bd, win, tid, x, dx);
    __syncthreads();
    for (int e = tid; e < pn * pn; e += MGT) add(pmap[e / pn], pmap[e % pn], Hp[e]);
    for (int i = tid; i < pn; i += MGT) {
      double sacc = b0[i];
      for (int q = 0; q < pn; ++q) sacc += Hp[(size_t)q * pn + i] * dx[q];
      const int t = loc(pmap[i]);
      if (t >= 0) b1[t] += sacc;
    }
    __syncthreads();
  }
  if (M.mode == 0) {
    // ---- IMULegFactor / IMUFactor between frames 0 and 1: whitened [J | r] staged through LDS ----
    if (M.has_imu) {
      const double *lin = bd.imu_lin + (size_t)win * 10 * 31 * 39;
      for (int e = tid; e < 31 * 39; e += MGT) tile[e] = lin[e];
      __syncthreads();
      for (int e = tid; e < 39 * 39; e += MGT) {
        const int a = e / 39, c = e % 39;
        if (a == 38) continue;
        double sacc = 0.0;
        for (int i = 0; i < 31; ++i) sacc += tile[i * 39 + a] * tile[i * 39 + c];
        auto cdof = [](int cc) { return cc < 6 ? cc : (cc < 19 ? CD_B0 + (cc - 6) : (cc < 25 ? 6 + (cc - 19) : CD_B0 + 13 + (cc - 25))); };
        if (c == 38) { const int t = loc(cdof(a)); if (t >= 0) b1[t] += sacc; }
        else add(cdof(a), cdof(c), sacc);
      }
      __syncthreads();
    }
    // ---- visual factors of the landmarks that start in frame 0: camera-side Gram slots of the s = 0 chunks ----
    for (int ch = 0; ch < wm.n_chunks; ++ch) {
      const ChunkMeta cm = bd.chunk[wm.chunk_off + ch];
      if (cm.s != 0) continue;
      for (int t = 0; t < cm.kmax; ++t) {
        const double *gs = bd.gram + (size_t)(cm.gram_off + t) * VILO_GRAM;
        for (int e = tid; e < VILO_GRAM26; e += MGT) {   // the 26-column view of the slot
          int a = 0, rem = e;
          while (rem >= 26 - a) { rem -= 26 - a; ++a; }
          const int bc = a + rem;
          if (t == 0 && ((a >= 6 && a < 12) || (bc >= 6 && bc < 12))) continue;
          auto cdof = [&](int c) { return c < 6 ? c : (c < 12 ? 6 * t + (c - 6) : (c < 18 ? CD_EX0 + c - 12 : (c < 24 ? CD_EX1 + c - 18 : CD_TD))); };
          double sg;
          const int ge = gram26_index(a, bc, sg);
          const double v = sg * gs[ge];
          if (bc == 25) { if (a < 25) { const int q = loc(cdof(a)); if (q >= 0) b1[q] += v; } }
          else {
            add(cdof(a), cdof(bc), v);
            if (cdof(a) != cdof(bc)) add(cdof(bc), cdof(a), v);
          }
        }
        __syncthreads();
      }
    }
  }
  stamp(1);
  // ---- certificate copy: C - eps I (dense dropped block before the landmarks are folded in) ----
  for (int e = tid; e < md * md; e += MGT) Ce[e] = A1[(e / md) * T + e % md] - ((e / md == e % md) ? eps : 0.0);
  // camera dims that exist in this problem (rows of the landmark coupling W)
  if (tid == 0) {
    int k = 0;
    for (int a = 0; a < 79; ++a) { const int t = loc(a); if (t >= 0) { act_a[k] = a; act_t[k] = t; ++k; } }
    n_act = k;
  }
  __syncthreads();
  // ---- eliminate the dropped landmarks: A1 -= W D^-1 W^T, b1 -= W D^-1 g, tile by tile ----
  if (L0 > 0) {
    const int na = n_act;
    const double *wl = bd.lm_w + 80 * (size_t)wm.lm_off;
    for (int l0 = 0; l0 < L0; l0 += MG_TILE) {
      const int nl = min(MG_TILE, L0 - l0);
      if (tid < nl) {
        const int l = drop_lm[(size_t)win * max_l0 + l0 + tid];
        const double D = bd.lm_E[wm.lm_off + l];
        if (!(D - eps > 0.0)) fail = 1;
        dinv[tid] = 1.0 / D; deps[tid] = 1.0 / (D - eps); gl[tid] = bd.lm_gbuf[0][wm.lm_off + l];
      }
      for (int e = tid; e < na * MG_TILE; e += MGT) {
        const int k = e / MG_TILE, j = e % MG_TILE;
        tile[e] = (j < nl) ? wl[(size_t)act_a[k] * wm.L + drop_lm[(size_t)win * max_l0 + l0 + j]] : 0.0;
      }
      __syncthreads();
      // W D^-1 W^T of the tile on the FP64 matrix cores: one 16 x 16 block of the (compact) active-dimension index per wave, K = the
      // 32 landmarks of the tile (8 k-steps); lane (lr, lk) supplies W[16 K1 + lr][4 kk + lk] / D and W[16 K2 + lr][4 kk + lk]
      {
        const int wv_ = tid >> 6, lane_ = tid & 63, lr = lane_ & 15, lk = lane_ >> 4;
        const int nb = (na + 15) >> 4;
        for (int blk = wv_; blk < (nb * (nb + 1)) / 2; blk += MGT / 64) {
          int K1 = 0;
          while (((K1 + 1) * (K1 + 2)) / 2 <= blk) ++K1;
          const int K2 = blk - (K1 * (K1 + 1)) / 2;
          const int ra = 16 * K1 + lr, rb = 16 * K2 + lr;
          mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int kk = 0; kk < MG_TILE / 4; ++kk) {
            const int j = 4 * kk + lk;
            const double wa = (ra < na && j < nl) ? tile[ra * MG_TILE + j] * dinv[j] : 0.0;
            const double wb = (rb < na && j < nl) ? tile[rb * MG_TILE + j] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wa, wb, acc, 0, 0, 0);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k1 = 16 * K1 + lk + 4 * r, k2 = 16 * K2 + lr;
            if (k1 < na && k2 < na && (K1 != K2 || k2 <= k1)) {
              const int t1 = act_t[k1], t2 = act_t[k2];
              A1[t1 * T + t2] -= acc[r];
              if (t1 != t2) A1[t2 * T + t1] -= acc[r];
            }
          }
        }
      }
      // the certificate's copy of the dense dropped block takes the same update with 1 / (D - eps)
      for (int e = tid; e < na * (na + 1) / 2; e += MGT) {
        int k1 = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
        while ((k1 + 1) * (k1 + 2) / 2 <= e) ++k1;
        while (k1 * (k1 + 1) / 2 > e) --k1;
        const int k2 = e - k1 * (k1 + 1) / 2;
        const int t1 = act_t[k1], t2 = act_t[k2];
        if (!(t1 < md && t2 < md)) continue;
        double se = 0.0;
        for (int j = 0; j < nl; ++j) se += tile[k1 * MG_TILE + j] * tile[k2 * MG_TILE + j] * deps[j];
        Ce[t1 * md + t2] -= se;
        if (t1 != t2) Ce[t2 * md + t1] -= se;
      }
      if (tid < na) {
        double sacc = 0.0;
        for (int j = 0; j < nl; ++j) sacc += tile[tid * MG_TILE + j] * gl[j] * dinv[j];
        b1[act_t[tid]] -= sacc;
      }
      __syncthreads();
    }
  }
  stamp(2);
  // ---- certificate: Amm - eps I positive definite <=> Cholesky of its landmark-reduced dense block has positive pivots ----
  chol_lds(Ce, md, md, &fail);
  if (fail) { if (tid == 0) need_general[win] = 1; return; }
  // ---- eliminate the dense dropped dims: A' = Arr - Arm C^-1 Amr with C = L L^T ----
  chol_lds(A1, T, md, &fail);
  if (fail) { if (tid == 0) need_general[win] = 1; return; }
  stamp(3);
  double *Y = tile;   // md x n, Y = L^-1 A1[0:md, md:T]
  if (tid <= n) {
    for (int i = 0; i < md; ++i) {
      double sacc = (tid < n) ? 0.5 * (A1[i * T + md + tid] + A1[(md + tid) * T + i]) : b1[i];
      for (int k = 0; k < i; ++k) sacc -= A1[i * T + k] * ((tid < n) ? Y[k * n + tid] : yb[k]);
      sacc /= A1[i * T + i];
      if (tid < n) Y[i * n + tid] = sacc; else yb[i] = sacc;
    }
  }
  __syncthreads();
  // A' = Arr - Y^T Y (lower triangle, mirrored: SelfAdjointEigenSolver reads the lower triangle) on the FP64 matrix cores: 16 x 16 blocks
  // of the kept dimensions, K = the <= 19 dense dropped dims (5 k-steps); the blocks stay in registers until every wave has read its part
  // of A1, then go to the compact layout (ld = MG_LD) that overlaps it
  constexpr int NBN = (MG_NMAX + 15) / 16, NBLK = (NBN * (NBN + 1)) / 2, BPW = (NBLK + MGT / 64 - 1) / (MGT / 64);
  mfma_d4 keep[BPW];
  {
    const int wv_ = tid >> 6, lane_ = tid & 63, lr = lane_ & 15, lk = lane_ >> 4;
    const int nbn = (n + 15) >> 4;
#pragma unroll
    for (int u = 0; u < BPW; ++u) {
      const int blk = wv_ + u * (MGT / 64);
      keep[u] = mfma_d4{0.0, 0.0, 0.0, 0.0};
      if (blk >= (nbn * (nbn + 1)) / 2) continue;
      int I = 0;
      while (((I + 1) * (I + 2)) / 2 <= blk) ++I;
      const int J = blk - (I * (I + 1)) / 2;
      mfma_d4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int kk = 0; kk < 5; ++kk) {
        const int k = 4 * kk + lk;
        const double ya = (k < md && 16 * I + lr < n) ? Y[k * n + 16 * I + lr] : 0.0;
        const double yc = (k < md && 16 * J + lr < n) ? Y[k * n + 16 * J + lr] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, yc, acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + lk + 4 * r, j = 16 * J + lr;
        keep[u][r] = (i < n && j < n && j <= i) ? A1[(md + i) * T + md + j] - acc[r] : 0.0;
      }
    }
  }
  if (tid < n) {
    double sacc = b1[md + tid];
    for (int k = 0; k < md; ++k) sacc -= Y[k * n + tid] * yb[k];
    br[tid] = sacc;
  }
  __syncthreads();
  double *Ar = ml, *V2 = ml + MG_NMAX * MG_LD;
  {
    const int wv_ = tid >> 6, lane_ = tid & 63, lr = lane_ & 15, lk = lane_ >> 4;
    const int nbn = (n + 15) >> 4;
#pragma unroll
    for (int u = 0; u < BPW; ++u) {
      const int blk = wv_ + u * (MGT / 64);
      if (blk >= (nbn * (nbn + 1)) / 2) continue;
      int I = 0;
      while (((I + 1) * (I + 2)) / 2 <= blk) ++I;
      const int J = blk - (I * (I + 1)) / 2;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + lk + 4 * r, j = 16 * J + lr;
        if (i < n && j < n && j <= i) { Ar[i * MG_LD + j] = keep[u][r]; Ar[j * MG_LD + i] = keep[u][r]; }
      }
    }
  }
  __syncthreads();
  stamp(4);
  double *J0 = J0_out + (size_t)win * VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM, *r0 = r0_out + (size_t)win * VILO_MAX_PRIOR_DIM;
  prior_factor_lds(Ar, V2, br, n, eps, cs, J0, r0, &status[win], clk ? clk + win * 8 : nullptr, factor_form != 0);
  stamp(6);
}

// flag[w] = the IMU factor of interval 0 is live and its covariance had no sqrt_info
__global__ void k_marg_imu0_bad(int W, const int *prep_bad, const unsigned char *imu_skip, int *flag) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < W) flag[w] = (!imu_skip[(size_t)w * 10] && prep_bad[(size_t)w * 10]) ? 1 : 0;
}

// new priors of pooled windows: device to device into their slot (n x n packed, ld n); src >= 0: the unchanged prior moves
// from slot src to slot dst (MARGIN_SECOND_NEW with nothing to drop)
__global__ void __launch_bounds__(256) k_prior_scatter(int W, const MargWin *mw, const int *dst, const int *src, const double *J0, const double *r0, double *pJ,
                                                       double *pr) {
  const int w = blockIdx.x;
  if (w >= W || dst[w] < 0) return;
  double *dj = pJ + (size_t)dst[w] * 96 * 96, *dr = pr + (size_t)dst[w] * 96;
  if (src[w] >= 0) {
    const double *sj = pJ + (size_t)src[w] * 96 * 96, *sr = pr + (size_t)src[w] * 96;
    for (int e = threadIdx.x; e < 96 * 96; e += 256) dj[e] = sj[e];
    for (int e = threadIdx.x; e < 96; e += 256) dr[e] = sr[e];
    return;
  }
  const int n = mw[w].n;
  const double *sj = J0 + (size_t)w * VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM, *sr = r0 + (size_t)w * VILO_MAX_PRIOR_DIM;
  for (int e = threadIdx.x; e < n * n; e += 256) dj[e] = sj[e];
  for (int e = threadIdx.x; e < n; e += 256) dr[e] = sr[e];
}

// What marg_run leaves for marg_store: the call's device blocks (BatchCall memory), the staging they went up from, the flags as last read
struct MargMem {
  char *hblob = nullptr;       // page-locked staging of the block that goes up: window tables | dropped landmarks | flags | pool slots
  MargWin *h_mw = nullptr, *d_mw = nullptr;
  int *h_slots = nullptr, *d_slots = nullptr;   // [2][W] prior-pool slots: destination, source
  int *d_flags = nullptr;      // [3][W] status | need_general | the IMU factor of interval 0 stands on a covariance without sqrt_info
  double *d_J0 = nullptr, *d_r0 = nullptr;
  size_t nJ0 = 0, nr0 = 0;
  std::vector<int> flags;      // d_flags on the host
};

// Step 1, no GPU: what each window's marginalisation drops and keeps (marg_plan.hpp), from the batch's landmark order and mask mirror and
// the windows' references
int marg_plan(vilo_batch *bt, int W, const vilo_window_desc *in, const vilo_resident_refs *refs, const int *modes, MargPlan &plan) {
  std::vector<MargWindow> win(W);
  for (int w = 0; w < W; ++w) {
    const vilo_resident_refs *rf = refs ? refs + w : nullptr;
    MargWindow &m = win[w];
    m.desc = in + w; m.mode = modes[w];
    if (m.mode < 0) continue;
    m.prior = vilo_win_prior(in[w], rf);
    if (m.mode == 0) m.sum_dt0 = vilo_win_sum_dt(in[w], rf, 0);
    m.L = bt->lm.L[w]; m.perm = bt->lm.perm.data() + bt->lm.lm_off[w]; m.mask = bt->mask.host(bt->lm.lm_off[w]);
  }
  return plan_marginalization(W, win.data(), plan).code;
}

// Behind the marginalisation's kernels on the stream: k_marg_imu0_bad folds its flag per window, the stream drains, the three rows of
// flags come back. launch_err: what vilo_last_error says of a launch or the stream that failed (null: nothing).
int marg_read_flags(vilo_ctx *ctx, const BatchDev &bd, int W, MargMem &mem, const char *launch_err) {
  if (bd.prep_bad) hipLaunchKernelGGL(k_marg_imu0_bad, dim3((W + 255) / 256), dim3(256), 0, ctx->stream, W, bd.prep_bad, bd.imu_skip, mem.d_flags + 2 * (size_t)W);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    if (launch_err) ctx->err = launch_err;
    return VILO_ERR_HIP;
  }
  if (hipMemcpy(mem.flags.data(), mem.d_flags, sizeof(int) * 3 * (size_t)W, hipMemcpyDeviceToHost) != hipSuccess) return VILO_ERR_HIP;
  return VILO_OK;
}

// VILO_MARG_CLOCKS: the phases of k_marginalize_lds on window 0
void marg_print_clocks(const long long *d_clk) {
  long long c[8];
  if (hipMemcpy(c, d_clk, sizeof(c), hipMemcpyDeviceToHost) == hipSuccess)
    fprintf(stderr, "[k_marginalize_lds] window 0 cycles: assemble %lld, landmarks %lld, cholesky %lld, schur %lld, pivoted cholesky %lld, jacobi %lld, output %lld\n", c[1] - c[0],
            c[2] - c[1], c[3] - c[2], c[4] - c[3], c[7] - c[4], c[5] - c[7], c[6] - c[5]);
}

// The windows marked general — rank-deficient Amm (or an over-sized problem) — through k_marginalize: thresholded eigen pseudo-inverse of
// the full Amm in global memory
int marg_run_general(BatchCall &call, BatchDev &bd, MargPlan &plan, MargMem &mem, const int *d_drop) {
  vilo_ctx *ctx = call.ctx;
  const int W = (int)plan.wins.size();
  const size_t scratch_total = assign_marg_scratch(plan.wins);
  // the updated window tables go up in stream order behind the first copy, from the same staging updated in place (with the forced
  // path that copy may still be reading it: whatever it reads, this one lands last)
  memcpy(mem.h_mw, plan.wins.data(), sizeof(MargWin) * (size_t)W);
  double *d_scr = (double *)call.scope->alloc(sizeof(double) * std::max<size_t>(1, scratch_total));   // (sized only now: an allocation of its own)
  if (!d_scr || hipMemcpyAsync(mem.d_mw, mem.h_mw, sizeof(MargWin) * (size_t)W, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
  hipLaunchKernelGGL(k_marginalize, dim3(W), dim3(MT), 0, ctx->stream, bd, mem.d_mw, d_drop, plan.max_l0, d_scr, mem.d_J0, mem.d_r0, mem.d_flags);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "k_marginalize launch failed"; return VILO_ERR_HIP; }
  return VILO_OK;
}

// Step 2: the plan's tables go up, the factors are linearised at the batch's state, k_marginalize_lds runs every window and k_marginalize
// those it hands on; J0 / r0 stay on the device, the flags are on the host when it returns.
int marg_run(BatchCall &call, MargPlan &plan, MargMem &mem) {
  vilo_ctx *ctx = call.ctx;
  BatchDev &bd = call.bt->d;
  const int W = (int)plan.wins.size();
  // The call's device memory (BatchCall: given back when the call returns) starts with one block for what goes up (window tables,
  // dropped-landmark lists, prior-pool slots) and the flags that come back (status, need_general, "the IMU factor of interval 0 stands on
  // a covariance without sqrt_info"): one upload, one download per call — a one-window call per image used to spend more time in its
  // dozen synchronous copies and allocations than in its kernels. Behind it J0, r0 and the clock stamps, which stay on the device.
  const bool want_clk = getenv("VILO_MARG_CLOCKS") != nullptr;
  const size_t off_mw = call.lay.take<MargWin>(W), off_drop = call.lay.take<int>(plan.drop_lm.size());
  const size_t off_flags = call.lay.take<int>(3 * (size_t)W), off_slots = call.lay.take<int>(2 * (size_t)W), blob_bytes = call.lay.bytes();
  mem.nJ0 = (size_t)W * VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM; mem.nr0 = (size_t)W * VILO_MAX_PRIOR_DIM;
  const size_t off_J0 = call.lay.take<double>(mem.nJ0), off_r0 = call.lay.take<double>(mem.nr0), off_clk = call.lay.take<long long>(8 * (size_t)W, want_clk);
  // (the context's reusable page-locked staging: the scope's closing sync outlives the asynchronous copies on every return path)
  mem.hblob = (char *)vilo_host_stage(ctx, 6, blob_bytes);
  if (!mem.hblob) return VILO_ERR_HIP;
  mem.h_mw = (MargWin *)(mem.hblob + off_mw); mem.h_slots = (int *)(mem.hblob + off_slots);
  memset(mem.hblob, 0, blob_bytes);
  memcpy(mem.h_mw, plan.wins.data(), sizeof(MargWin) * (size_t)W);
  if (!plan.drop_lm.empty()) memcpy(mem.hblob + off_drop, plan.drop_lm.data(), sizeof(int) * plan.drop_lm.size());
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  mem.d_J0 = call.ptr<double>(off_J0); mem.d_r0 = call.ptr<double>(off_r0);
  long long *d_clk = want_clk ? call.ptr<long long>(off_clk) : nullptr;
  mem.d_mw = call.ptr<MargWin>(off_mw);   // (the first block: the blob starts here)
  mem.d_flags = call.ptr<int>(off_flags); mem.d_slots = call.ptr<int>(off_slots);
  int *d_drop = call.ptr<int>(off_drop), *d_status = mem.d_flags, *d_general = mem.d_flags + W;
  if (hipMemcpyAsync(mem.d_mw, mem.hblob, blob_bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
  // preMarginalize: evaluate the factors at the current state (marginalization_factor.cpp:119-138)
  VILO_HIP(call.start());
  int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  const size_t lds_bytes = (size_t)MG_LDS_DOUBLES * sizeof(double);
  if (!ctx->marg_attr_set) {   // (per context = per device and host thread)
    if (hipFuncSetAttribute((const void *)k_marginalize_lds, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes) != hipSuccess) return VILO_ERR_HIP;
    ctx->marg_attr_set = true;
  }
  const bool force_general = getenv("VILO_MARG_GENERAL") != nullptr;   // test hook: every window through the global-memory eigen path
  mem.flags.assign(3 * (size_t)W, 0);
  if (!force_general) {
    hipLaunchKernelGGL(k_marginalize_lds, dim3(W), dim3(MGT), lds_bytes, ctx->stream, bd, mem.d_mw, d_drop, plan.max_l0, mem.d_J0, mem.d_r0, d_status, d_general, d_clk,
                       ctx->prior_form);
    rc = marg_read_flags(ctx, bd, W, mem, "k_marginalize_lds launch failed");
    if (rc != VILO_OK) return rc;
    if (want_clk) marg_print_clocks(d_clk);
  }
  ctx->marg_general_count = 0;
  for (int w = 0; w < W; ++w)
    if ((force_general || mem.flags[(size_t)W + w]) && plan.wins[w].m > 0 && plan.wins[w].n > 0) { plan.wins[w].general = 1; ++ctx->marg_general_count; }
  if (ctx->marg_general_count > 0) {
    rc = marg_run_general(call, bd, plan, mem, d_drop);
    if (rc != VILO_OK) return rc;
  }
  VILO_HIP(call.finish());
  // (k_marginalize writes status too, and the forced path has read nothing yet)
  if (force_general || ctx->marg_general_count > 0) return marg_read_flags(ctx, bd, W, mem, nullptr);
  return VILO_OK;
}

// Windows with a prior pool leave J0 / r0 on the device (slot next_prior_slot): k_prior_scatter moves them there, or the unchanged prior
// from its old slot; only their kept-block bookkeeping is host side. any_host: some window's prior goes back to host memory.
int marg_scatter_pooled(vilo_ctx *ctx, const MargPlan &plan, MargMem &mem, const vilo_resident_refs *refs, const std::vector<int> &status, bool *any_host) {
  const int W = (int)plan.wins.size();
  std::vector<int> dst_slot(W, -1), src_slot(W, -1);
  for (int w = 0; w < W; ++w) {
    if (plan.skip[w]) continue;
    if (refs && refs[w].prior_pool) {
      vilo_prior_pool *pl = refs[w].prior_pool;
      if (refs[w].next_prior_slot < 0 || refs[w].next_prior_slot >= pl->n) return VILO_ERR_BAD_ARG;
      if (plan.keep_prior[w]) { if (refs[w].prior_slot != refs[w].next_prior_slot) src_slot[w] = refs[w].prior_slot; else continue; }
      else if (status[w] || plan.wins[w].m == 0 || plan.wins[w].n == 0) continue;   // (no prior comes out of this window: its slot is left alone, meta.valid cleared by the caller)
      dst_slot[w] = refs[w].next_prior_slot;
    } else {
      *any_host = true;
    }
  }
  if (refs && refs[0].prior_pool) {
    int *h_slots = mem.h_slots;   // (the stream has drained: no copy reads the staging any more)
    memcpy(h_slots, dst_slot.data(), sizeof(int) * W);
    memcpy(h_slots + W, src_slot.data(), sizeof(int) * W);
    if (hipMemcpyAsync(mem.d_slots, h_slots, sizeof(int) * 2 * (size_t)W, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return VILO_ERR_HIP;
    hipLaunchKernelGGL(k_prior_scatter, dim3(W), dim3(256), 0, ctx->stream, W, mem.d_mw, mem.d_slots, mem.d_slots + W, mem.d_J0, mem.d_r0, refs[0].prior_pool->dJ,
                       refs[0].prior_pool->dr);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) return VILO_ERR_HIP;
  }
  return VILO_OK;
}

// Step 3: every window's new prior, into its pool slot or out[w]
int marg_store(vilo_ctx *ctx, const BatchDev &bd, const MargPlan &plan, MargMem &mem, const vilo_window_desc *in, const vilo_resident_refs *refs,
               const vilo_window_state *state, vilo_prior *out) {
  const int W = (int)plan.wins.size();
  // Status first: a window whose result is unusable must not overwrite a pool slot either.
  std::vector<int> status(mem.flags.begin(), mem.flags.begin() + W);
  // A preintegration covariance that is not positive definite has no sqrt_info (its bad pivots were replaced by 1 so that the arithmetic
  // stays finite): an IMU factor built on it would give a finite but meaningless prior. Only the factors that ENTER this marginalisation
  // count — MARGIN_OLD uses the factor of interval 0 alone (estimator.cpp:1271-1297), MARGIN_SECOND_NEW no IMU factor at all
  // (:1389-1410) —, like the reference, which would yield a valid prior whatever the other intervals look like. The flags are those of
  // the records in force: written by the preparation (batch creation / vilo_batch_prepare) or, with re-propagation, by the mode-0 pass
  // of the linearisation (k_marg_imu0_bad folds them per window behind the marginalisation's kernels). Treated like a non-finite result:
  // the window goes on without a prior and the call reports VILO_ERR_NUMERIC.
  if (bd.prep_bad)
    for (int w = 0; w < W; ++w)
      if (!plan.skip[w] && plan.wins[w].mode == 0 && mem.flags[2 * (size_t)W + w]) status[w] = 1;
  bool any_host = false;
  const int rc = marg_scatter_pooled(ctx, plan, mem, refs, status, &any_host);
  if (rc != VILO_OK) return rc;
  // priors that go back to host memory: through the context's reusable page-locked staging (a fresh pageable vector of W x 74 KB was
  // zero-filled, then filled again through the runtime's bounce buffer: most of a fleet's marginalisation call)
  const double *J0 = nullptr, *r0 = nullptr;
  if (any_host) {
    double *hJ = (double *)vilo_host_stage(ctx, 7, sizeof(double) * (mem.nJ0 + mem.nr0));
    if (!hJ) return VILO_ERR_HIP;
    if (hipMemcpyAsync(hJ, mem.d_J0, mem.nJ0 * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipMemcpyAsync(hJ + mem.nJ0, mem.d_r0, mem.nr0 * 8, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
      return VILO_ERR_HIP;
    J0 = hJ; r0 = hJ + mem.nJ0;
  }
  int any_bad = 0;
  for (int w = 0; w < W; ++w) {
    const MargWin &M = plan.wins[w];
    if (plan.skip[w]) continue;
    const bool pooled = refs && refs[w].prior_pool;
    vilo_prior &p = pooled ? refs[w].prior_pool->meta[refs[w].next_prior_slot] : out[w];
    if (plan.keep_prior[w]) { copy_prior_meta(*vilo_win_prior(in[w], refs ? refs + w : nullptr), p, pooled); continue; }
    if (M.m == 0 || M.n == 0) { p.valid = 0; p.n = 0; continue; }
    // a non-finite result concerns this window alone: it goes on without a prior, the others keep theirs (the call still reports it)
    if (status[w]) { p.valid = 0; p.n = 0; any_bad = 1; continue; }
    write_prior_meta(plan, w, in[w].n_frames, state[w], p);
    if (pooled) continue;
    memcpy(p.J0, J0 + (size_t)w * VILO_MAX_PRIOR_DIM * VILO_MAX_PRIOR_DIM, sizeof(double) * (size_t)M.n * M.n);   // (n x n packed on both sides)
    memcpy(p.r0, r0 + (size_t)w * VILO_MAX_PRIOR_DIM, sizeof(double) * M.n);
  }
  if (any_bad) { ctx->err = "non-finite marginalisation result (the windows concerned continue without a prior)"; return VILO_ERR_NUMERIC; }
  return VILO_OK;
}

}  // namespace

extern "C" double vilo_last_marginalize_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_marg_ms : 0.0; }
extern "C" int vilo_debug_marg_general_count(const vilo_ctx *ctx) { return ctx ? ctx->marg_general_count : 0; }

// Every return below the BatchCall happens while it is alive: its closing synchronisation is what makes the asynchronous copies out of
// the staging safe.
int vilo_marginalize_batch(vilo_ctx *ctx, vilo_batch *bt, int W, const vilo_window_desc *in, const vilo_resident_refs *refs, const vilo_window_state *state,
                           const int *modes, vilo_prior *out) {
  if (bt->mask.stale(ctx, "vilo_batch_marginalize") != VILO_OK) return VILO_ERR_HIP;
  MargPlan plan;
  int rc = marg_plan(bt, W, in, refs, modes, plan);
  if (rc != VILO_OK) return rc;
  BatchCall call(ctx, bt, &vilo_ctx::last_marg_ms);
  MargMem mem;
  rc = marg_run(call, plan, mem);
  if (rc != VILO_OK) return rc;
  return marg_store(ctx, bt->d, plan, mem, in, refs, state, out);
}

extern "C" int vilo_marginalize(vilo_ctx *ctx, int W, const vilo_window_desc *in, const vilo_window_state *state, int mode,
                                vilo_prior *out) {
  if (!ctx || W <= 0 || !in || !state || !out || (mode != 0 && mode != 1)) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  std::vector<int> modes(W, mode);
  return vilo_with_batch(ctx, W, in, state, [&](vilo_batch *bt) { return vilo_marginalize_batch(ctx, bt, W, in, nullptr, state, modes.data(), out); });
}

// The marginalisation half on a batch that is already resident (after vilo_batch_solve + vilo_batch_download): linearised at the batch's
// device state; `state` is the host copy of it (keep_block_data of the new prior). modes[w]: 0 MARGIN_OLD, 1 MARGIN_SECOND_NEW, < 0 skip.
extern "C" int vilo_batch_marginalize(vilo_ctx *ctx, vilo_batch *bt, int W, const vilo_window_desc *in, const vilo_window_state *state, const int *modes,
                                      vilo_prior *out) {
  if (!ctx || !bt || W <= 0 || W != bt->d.W || !in || !state || !modes || !out) return VILO_ERR_BAD_ARG;
  for (int w = 0; w < W; ++w)
    if (modes[w] > 1) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  return vilo_marginalize_batch(ctx, bt, W, in, nullptr, state, modes, out);
}
