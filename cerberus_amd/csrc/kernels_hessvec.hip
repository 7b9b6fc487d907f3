// Gauss-Newton Hessian-vector products of every window of a batch at its current device state (vilo_batch_hessian_vector, include/vilo_gpu.h).
//
// Linearisation: the marginalisation's pass (vilo_marg_linearize, mode 0), exactly as vilo_batch_gradient and vilo_batch_gauss_newton_step
// run it: the windows' SolverStates are copied aside before and back after; x, lambda and the prior are only read.
//
// k_hess_vec, one workgroup per window, one code path for every batch size and every K, all FP64, no floating-point atomics. The K vectors
// of a window are the columns of V [224 camera dimensions (solver_types.hpp) + L][16], columns K .. 15 zero; entries of constant blocks and
// absent frames are zero and never read from the caller's arrays. H is never assembled beyond the 80 x 80 pose block of the visual factors:
// every other source is applied to its own slice of V. Steps, every product on v_mfma_f64_16x16x4f64 (operand placement of step_syrk_wave /
// k_landmark_covariance: lane (lr, lk) gives A[row lr][k lk] and B[k lk][column lr], accumulator r is row lk + 4 r, column lr):
//   1. g of the 222 state entries by their owners (state_entry_gh of gn_system.hpp, without the diagonal; the record's g . v).
//   2. V into LDS by camera dimension; a read entry that is not finite marks its column (status 1) and is taken as 0.
//   3. P = the visual Gram slots' 80 x 80 block (assemble_visual_pose_block of gn_system.hpp); Y_P = P V_P (5 row tiles, 20 k-steps).
//   4. the IMU Gram of every interval k, 38 x 38 over [pose_k 6 | B_k 13 | pose_k+1 6 | B_k+1 13], applied to those rows of V and added to
//      those rows of Y (3 row tiles, 10 k-steps; intervals in ascending order, a barrier between them): the speed / bias chain and the
//      143 x 80 coupling are never materialised.
//   5. the prior's H (pn x pn, pn <= 96) applied to the rows prior_map names, added to those rows of Y (6 row tiles at the most).
//   6. the landmarks, 32 per pass, lm_w read once for all columns: the pass's coupling rows w_l [79] and v_l [16] are staged in LDS;
//      Y_P += sum_l w_l v_l on the matrix cores (accumulators kept in registers over the passes), y_l = E_l v_l + w_l^T v_P by thread
//      (landmark, column pair), written to the caller's order (lm_off + lm_perm).
//   7. the record of every column: thread (i, column pair) takes the landmarks i, i + 32, ... and the camera dimensions i, i + 32, ...,
//      then one thread per column adds the 32 partial sums in ascending order.
// A column's arithmetic does not depend on the other columns, on its own index or on K (the unused columns are zero operands).
// LDS: P 51 200 B (the landmark staging, 25 216 B, and the record's partial sums, 8448 B, reuse it once P V_P is done) + V 28 672 B + Y
// 28 672 B + g 1792 B + prior dx 768 B + maps 896 B = 112 000 B: one workgroup per CU (DESIGN 4.28 has the decision).
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "gn_system.hpp"

static_assert(sizeof(vilo_hess_vec_record) == 32, "vilo_hess_vec_record: 32 bytes (cerberus_amd/_ctypes.py mirrors it)");
static_assert(VILO_HV_MAX_VECTORS == 16, "k_hess_vec: one 16-column tile of v_mfma_f64_16x16x4f64");

#define HV_K 16             // columns of a tile (VILO_HV_MAX_VECTORS)
#define HV_LMC 32           // landmarks per pass
#define HV_WS 33            // row stride of the staged coupling rows (a pad of one: the tile's 16 rows fall into 16 banks)
// LDS (doubles)
#define HL_P 0                                // [80][80] visual pose block; then: staging | partial sums
#define HL_WT HL_P                            //   [80][33] w_l of a pass, by camera dimension
#define HL_VL (HL_WT + GN_NP * HV_WS)         //   [32][16] v_l of a pass
#define HL_RED HL_P                           //   [2][16][33] partial sums of v . Hv and g . v
#define HL_V (HL_P + GN_NP * GN_NP)           // [224][16] V by camera dimension
#define HL_Y (HL_V + CD_N * HV_K)             // [224][16] Y
#define HL_G (HL_Y + CD_N * HV_K)             // [224] g by camera dimension
#define HL_DX (HL_G + CD_N)                   // [96] prior dx
#define HL_MAP (HL_DX + VILO_MAX_PRIOR_DIM)   // int pmap[96], short inv_pmap[224], int badk[16]
#define HL_N (HL_MAP + (96 * 4 + 224 * 2 + 16 * 4 + 7) / 8)
static_assert(HL_VL + HV_LMC * HV_K <= HL_V && 2 * HV_K * HV_WS <= GN_NP * GN_NP, "k_hess_vec: what reuses P's place");
static_assert(sizeof(double) * HL_N <= 160 * 1024, "k_hess_vec: the CU's LDS");

__global__ void __launch_bounds__(GN_T) k_hess_vec(BatchDev b, int K, const double *sv_in, const double *lv_in, vilo_hess_vec_record *rec, double *ss_out,
                                                  double *ls_out) {
  using namespace vilo;
  extern __shared__ double lds[];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, lr = lane & 15, lk = lane >> 4;
  const WinMeta wm = b.win[w];
  const int F = wm.n_frames, L = wm.L;
  double *Pm = lds + HL_P, *Wt = lds + HL_WT, *Vl = lds + HL_VL, *red = lds + HL_RED, *Vs = lds + HL_V, *Ys = lds + HL_Y, *gs = lds + HL_G, *dxs = lds + HL_DX;
  int *pmap = (int *)(lds + HL_MAP);
  short *inv_pmap = (short *)(pmap + 96);
  int *badk = (int *)(inv_pmap + CD_N);
  double *so = ss_out ? ss_out + (size_t)w * K * GN_NS : nullptr, *lo = ls_out ? ls_out + (size_t)K * wm.lm_off : nullptr;
  const double *sv = sv_in ? sv_in + (size_t)w * K * GN_NS : nullptr, *lv = lv_in ? lv_in + (size_t)K * wm.lm_off : nullptr;
  if (b.win_bad && b.win_bad[w]) {   // a record without sqrt_info: the window is not linearised
    if (so) for (int e = tid; e < K * GN_NS; e += GN_T) so[e] = NAN;
    if (lo) for (int e = tid; e < K * L; e += GN_T) lo[e] = NAN;
    if (rec && tid < K) {
      vilo_hess_vec_record r;
      r.vHv = NAN; r.g_dot_v = NAN; r.model_cost_change = NAN; r.status = 2; r.pad = 0;
      rec[(size_t)w * K + tid] = r;
    }
    return;
  }
  const int pn = wm.prior_n;
  for (int e = tid; e < GN_NP * GN_NP; e += GN_T) Pm[e] = 0.0;
  for (int e = tid; e < CD_N * HV_K; e += GN_T) { Vs[e] = 0.0; Ys[e] = 0.0; }
  for (int e = tid; e < CD_N; e += GN_T) gs[e] = 0.0;
  if (tid < HV_K) badk[tid] = 0;
  if (tid < 96) pmap[tid] = tid < pn ? b.prior_map[(size_t)w * 96 + tid] : 0;
  prior_view_init(b, wm, w, pmap, dxs, inv_pmap);

  // ---- 1. g of the 222 state entries ----
  if (tid < GN_NS) {
    const int cd = caller_cd(tid);
    if (cd_active(cd, F, wm.const_mask)) {
      double g = 0.0, h = 0.0;   // (h: not formed)
      state_entry_gh<false>(b, wm, w, cd, inv_pmap, dxs, g, h);
      gs[cd] = g;
    }
  }

  // ---- 2. V by camera dimension; the landmark entries are only checked here (they are staged pass by pass) ----
  // (badk[k] = 1 is stored by many threads, and again in step 7: benign, every writer stores the same value and barriers separate
  // the stores from the reads)
  if (sv)
    for (int e = tid; e < K * GN_NS; e += GN_T) {
      const int k = e / GN_NS, cd = caller_cd(e - k * GN_NS);
      if (!cd_active(cd, F, wm.const_mask)) continue;
      const double v = sv[e];
      if (isfinite(v)) Vs[cd * HV_K + k] = v;
      else badk[k] = 1;
    }
  if (lv)
    for (int e = tid; e < K * L; e += GN_T)
      if (!isfinite(lv[e])) badk[e / L] = 1;

  // ---- 3. P of the visual factors, Y_P = P V_P ----
  assemble_visual_pose_block(b, wm, Pm);
  __syncthreads();
  for (int X = wave; X < 5; X += 4) {   // (wave-uniform; P is symmetric: read down a column, lane by lane)
    const mfma_d4 acc = hv_tile(16 * X, GN_NP / 4, lr, lk, [&](int i, int kk) { return Pm[kk * GN_NP + i]; }, [&](int kk, int c) { return Vs[kk * HV_K + c]; });
#pragma unroll
    for (int r = 0; r < 4; ++r) Ys[(16 * X + lk + 4 * r) * HV_K + lr] = acc[r];
  }
  __syncthreads();

  // ---- 4. the IMU Grams, interval by interval ----
  for (int k = 0; k + 1 < F && k < VILO_WINDOW_SIZE; ++k) {
    if (b.imu_skip[w * 10 + k]) continue;   // (uniform)
    if (wave < 3) {
      const double *gr = b.imu_gram + (size_t)(w * 10 + k) * 780;
      const mfma_d4 acc = hv_tile(16 * wave, 10, lr, lk,
                                  [&](int i, int kk) { return (i < 38 && kk < 38) ? gr[tri39(min(i, kk), max(i, kk))] : 0.0; },
                                  [&](int kk, int c) { return kk < 38 ? Vs[hv_imu_cd(k, kk) * HV_K + c] : 0.0; });
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * wave + lk + 4 * r;
        if (row < 38) Ys[hv_imu_cd(k, row) * HV_K + lr] += acc[r];
      }
    }
    __syncthreads();
  }

  // ---- 5. the prior ----
  if (pn > 0) {
    const double *Hp = b.prior_H + (size_t)w * 96 * 96;
    for (int X = wave; 16 * X < pn; X += 4) {
      const mfma_d4 acc = hv_tile(16 * X, (pn + 3) / 4, lr, lk, [&](int i, int kk) { return (i < pn && kk < pn) ? Hp[(size_t)kk * pn + i] : 0.0; },
                                  [&](int kk, int c) { return kk < pn ? Vs[pmap[kk] * HV_K + c] : 0.0; });
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * X + lk + 4 * r;
        if (row < pn) Ys[pmap[row] * HV_K + lr] += acc[r];
      }
    }
  }
  __syncthreads();   // (P is done with: its place is the landmark staging below)

  // ---- 6. the landmarks ----
  const int li = tid & 31, c0 = 2 * (tid >> 5);
  double a_vhv[2] = {0.0, 0.0}, a_gv[2] = {0.0, 0.0};
  {
    const double *wl = b.lm_w + 80 * (size_t)wm.lm_off, *lmg = b.lm_gbuf[0] + wm.lm_off, *lmE = b.lm_E + wm.lm_off;
    const int *perm = b.lm_perm + wm.lm_off;
    mfma_d4 accP[2] = {mfma_d4{0.0, 0.0, 0.0, 0.0}, mfma_d4{0.0, 0.0, 0.0, 0.0}};   // tile `wave` of Y_P; wave 0: tile 4 too
    for (int l0 = 0; l0 < L; l0 += HV_LMC) {
      const int nl = min(HV_LMC, L - l0);
      for (int e = tid; e < GN_NP * HV_LMC; e += GN_T) {
        const int l = e % HV_LMC, a = e / HV_LMC;
        Wt[a * HV_WS + l] = (l < nl && a < VILO_NPU) ? wl[(size_t)a * L + l0 + l] : 0.0;
      }
      for (int e = tid; e < HV_LMC * HV_K; e += GN_T) {
        const int l = e / HV_K, c = e % HV_K;
        double v = 0.0;
        if (lv && l < nl && c < K) {
          v = lv[(size_t)c * L + perm[l0 + l]];
          if (!isfinite(v)) v = 0.0;
        }
        Vl[e] = v;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int X = wave + 4 * i;
        if (X < 5) {   // (wave-uniform)
          for (int ks = 0; ks < HV_LMC / 4; ++ks) {
            const int kk = 4 * ks + lk;
            accP[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wt[(16 * X + lr) * HV_WS + kk], Vl[kk * HV_K + lr], accP[i], 0, 0, 0);
          }
        }
      }
      if (li < nl) {
        const int l = l0 + li;
        const double E = lmE[l], gl = lmg[l];
        double y[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) y[j] = E * Vl[li * HV_K + c0 + j];
        for (int a = 0; a < VILO_NPU; ++a) {
          const double wv = Wt[a * HV_WS + li];
#pragma unroll
          for (int j = 0; j < 2; ++j) y[j] = fma(wv, Vs[a * HV_K + c0 + j], y[j]);
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const double v = Vl[li * HV_K + c0 + j];
          a_vhv[j] = fma(v, y[j], a_vhv[j]);
          a_gv[j] = fma(gl, v, a_gv[j]);
          if (lo && c0 + j < K) lo[(size_t)(c0 + j) * L + perm[l]] = y[j];
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int X = wave + 4 * i;
      if (X < 5) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Ys[(16 * X + lk + 4 * r) * HV_K + lr] += accP[i][r];
      }
    }
  }
  __syncthreads();

  // ---- 7. the records, then the state outputs ----
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double s_vhv = a_vhv[j], s_gv = a_gv[j];
    for (int cd = li; cd < CD_N; cd += 32) {
      const double v = Vs[cd * HV_K + c0 + j];
      s_vhv = fma(v, Ys[cd * HV_K + c0 + j], s_vhv);
      s_gv = fma(gs[cd], v, s_gv);
    }
    red[(c0 + j) * HV_WS + li] = s_vhv;
    red[(HV_K + c0 + j) * HV_WS + li] = s_gv;
  }
  __syncthreads();
  if (tid < K) {
    double vhv = 0.0, gv = 0.0;
    for (int i = 0; i < 32; ++i) { vhv += red[tid * HV_WS + i]; gv += red[(HV_K + tid) * HV_WS + i]; }
    const bool bad = badk[tid] != 0 || !isfinite(vhv) || !isfinite(gv);
    if (bad) badk[tid] = 1;
    if (rec) {
      vilo_hess_vec_record r;
      r.vHv = bad ? NAN : vhv;
      r.g_dot_v = bad ? NAN : gv;
      r.model_cost_change = bad ? NAN : -gv - 0.5 * vhv;
      r.status = bad ? 1 : 0;
      r.pad = 0;
      rec[(size_t)w * K + tid] = r;
    }
  }
  __syncthreads();
  if (so)
    for (int e = tid; e < K * GN_NS; e += GN_T) {
      const int k = e / GN_NS, cd = caller_cd(e - k * GN_NS);
      so[e] = !cd_active(cd, F, wm.const_mask) ? 0.0 : (badk[k] ? NAN : Ys[cd * HV_K + k]);
    }
  if (lo)
    for (int e = tid; e < K * L; e += GN_T)
      if (badk[e / L]) lo[e] = NAN;
}

extern "C" double vilo_last_hess_vec_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_hess_vec_ms : -1.0; }

extern "C" int vilo_batch_hessian_vector(vilo_ctx *ctx, vilo_batch *bt, int n_vec, const double *state_vec, const double *lm_vec, vilo_hess_vec_record *records,
                                         double *state_out, double *lm_out) {
  if (!ctx || !bt || !records) return VILO_ERR_BAD_ARG;
  if (n_vec < 1 || n_vec > VILO_HV_MAX_VECTORS) {
    ctx->err = "vilo_batch_hessian_vector: 1 <= n_vec <= VILO_HV_MAX_VECTORS (16) is required";
    return VILO_ERR_BAD_ARG;
  }
  if (bt->mask.refuse(ctx, "vilo_batch_hessian_vector") != VILO_OK) return VILO_ERR_UNSUPPORTED;
  BatchDev &bd = bt->d;
  const int W = bd.W, n_lm = bd.n_lm, K = n_vec;
  const size_t n_ss = (size_t)W * K * GN_NS, n_ls = (size_t)K * n_lm;
  BatchCall call(ctx, bt, &vilo_ctx::last_hess_vec_ms);
  // the call's device memory: saved solver state | records | state vectors | landmark vectors | state products | landmark products
  const size_t o_st = call.lay.take<SolverState>(W), o_rec = call.lay.take<vilo_hess_vec_record>((size_t)W * K);
  const size_t o_sv = call.lay.take<double>(n_ss, state_vec != nullptr), o_lv = call.lay.take<double>(n_ls, lm_vec != nullptr && n_ls > 0);
  const size_t o_ss = call.lay.take<double>(n_ss, state_out != nullptr), o_ls = call.lay.take<double>(n_ls, lm_out != nullptr && n_ls > 0);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  if (!ctx->hv_attr_set) {
    VILO_HIP(hipFuncSetAttribute((const void *)k_hess_vec, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(sizeof(double) * HL_N)));
    ctx->hv_attr_set = true;
  }
  if (state_vec) VILO_HIP(hipMemcpy(call.ptr<double>(o_sv), state_vec, sizeof(double) * n_ss, hipMemcpyHostToDevice));
  if (lm_vec && n_ls) VILO_HIP(hipMemcpy(call.ptr<double>(o_lv), lm_vec, sizeof(double) * n_ls, hipMemcpyHostToDevice));
  VILO_HIP(call.start());
  SolverStateGuard keep(call, bd, o_st);
  VILO_HIP(keep.saved);
  const int rc = vilo_marg_linearize(ctx, bd);
  if (rc != VILO_OK) return rc;
  hipLaunchKernelGGL(k_hess_vec, dim3(W), dim3(GN_T), sizeof(double) * HL_N, ctx->stream, bd, K, state_vec ? call.ptr<double>(o_sv) : (const double *)nullptr,
                     (lm_vec && n_ls) ? call.ptr<double>(o_lv) : (const double *)nullptr, call.ptr<vilo_hess_vec_record>(o_rec),
                     state_out ? call.ptr<double>(o_ss) : (double *)nullptr, (lm_out && n_ls) ? call.ptr<double>(o_ls) : (double *)nullptr);
  VILO_HIP(hipGetLastError());
  VILO_HIP(keep.restore());
  VILO_HIP(call.finish());
  VILO_HIP(call.down(records, call.ptr<char>(o_rec), sizeof(vilo_hess_vec_record) * (size_t)W * K));
  VILO_HIP(call.down(state_out, call.ptr<char>(o_ss), sizeof(double) * n_ss));
  VILO_HIP(call.down(lm_out, call.ptr<char>(o_ls), sizeof(double) * n_ls));
  return VILO_OK;
}

extern "C" int vilo_window_hessian_vector(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state, int n_vec,
                                          const double *state_vec, const double *lm_vec, vilo_hess_vec_record *records, double *state_out, double *lm_out) {
  if (!ctx || n_windows < 1 || !in || !state || !records) return VILO_ERR_BAD_ARG;
  return vilo_with_batch(ctx, n_windows, in, state,
                         [&](vilo_batch *bt) { return vilo_batch_hessian_vector(ctx, bt, n_vec, state_vec, lm_vec, records, state_out, lm_out); });
}
