// The host half of vilo_batch_leg_dead_reckon_covariance (include/vilo_gpu.h, kernels_legdrcov.hip): everything that needs no device. The
// argument checks, the sizes of the call's blocks, the embedding E of a 19 x 19 frame block into the 31 error coordinates, the noise
// diagonal of a step under the three contact models, the blocks of F and V of a step (imu_leg_integration_base.cpp:376-465 in the world
// frame), the two products of the recurrence, and the CPU path of one window. The nominal state is legdr_host.hpp's legdr_step, called,
// not restated. The samples are packed by leg_dead_reckon_pack and the step offsets formed by dead_reckon_step_offsets.
//
// A step's F and V are built into one block of doubles (LDC_SB_*), the kernel's in LDS, the CPU path's on the stack:
//   dF [21][16]  F - I without what is zero in every step: the rows dp dtheta dv deps (0 .. 20; the bias rows of F are unit rows) and the
//                columns dtheta dv (3 .. 8) and dba dbg drho (21 .. 30) (the dp and deps columns of F are unit columns)
//   W  [21][24]  the same rows of V at the noise columns that reach more than one row: acc_0 gyr_0 acc_1 gyr_1 phi_0 phi_1 dphi_0 dphi_1
//   qd [24]      their variances
//   nd [32]      what V Q V^T adds to the diagonal through V's -dt I blocks: dt^2 acc_w^2, dt^2 gyr_w^2, dt^2 rho_uncertainty
//   ne [4][9]    what it adds to the (deps_j, deps_j) block through V's -dt R_f block: dt^2 R_f diag(uncertainties_j) R_f^T. The
//                uncertainties are per axis of frame f's body frame (n_xy is not n_z), so in the world frame the block is not diagonal
//   terms        per leg and endpoint what the leg's rows need of a sample: v, p = p_br + R_br fk, h before its rotation, R_br J, g before
//                its rotation and sign (LDC_T_*); a sample is the second endpoint of one step and the first of the next: two slots
// Who writes what is the callers' business: the owner of leg j writes ldc_leg_rows(j) and ldc_leg_noise(j), the first one ldc_imu_rows.
// Sigma is held by columns: c <- F c is ldc_f_times (entries of dF that are zero in every step are not multiplied), Sigma' = F (F Sigma)^T
// takes a transposition between two of them, and ldc_add_noise adds column j of V Q V^T. The products name their fused multiply-adds, so
// the kernel and the CPU path round alike. HIP-free when compiled by a host compiler (tests/host_check/leg_dr_cov_check.cpp).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "legdr_host.hpp"

#if defined(__HIPCC__)
#define LDC_UNROLL _Pragma("unroll")   // a column of Sigma lives in registers: no loop over it may stay a loop
#else
#define LDC_UNROLL
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define LDC_ROW_DONE __builtin_amdgcn_sched_barrier(0);   // a row's block entries are loaded for that row, not for all rows ahead
#else
#define LDC_ROW_DONE
#endif

namespace vilo {

#define LDC_N 31        // error coordinates, ILStateOrder (parameters.h:135-149): dp dtheta dv deps_1..4 dba dbg drho_1..4
#define LDC_IN 19       // a frame block of vilo_batch_covariance: dp dtheta dv dba dbg drho
#define LDC_POSE 6      // the pose block of a pose_cov_trajectory row
#define LDC_LEGCOV 36   // doubles of a leg_cov_trajectory row: [4][3][3]
#define LDC_NOISE 46    // the reference's noise dimensions
#define LDC_ROWS 21
#define LDC_FK 16
#define LDC_WK 24
enum { LDC_O_P = 0, LDC_O_R = 3, LDC_O_V = 6, LDC_O_EPS = 9, LDC_O_BA = 21, LDC_O_BG = 24, LDC_O_RHO = 27 };
// compact columns of dF and of W
enum { LDC_K_R = 0, LDC_K_V = 3, LDC_K_BA = 6, LDC_K_BG = 9, LDC_K_RHO = 12 };
enum { LDC_W_A0 = 0, LDC_W_G0 = 3, LDC_W_A1 = 6, LDC_W_G1 = 9, LDC_W_PHI0 = 12, LDC_W_PHI1 = 15, LDC_W_DPHI0 = 18, LDC_W_DPHI1 = 21 };
enum { LDC_T_V = 0, LDC_T_P = 3, LDC_T_H = 6, LDC_T_J = 15, LDC_T_G = 24, LDC_T_N = 27 };
enum {
  LDC_SB_DF = 0,
  LDC_SB_W = LDC_SB_DF + LDC_ROWS * LDC_FK,
  LDC_SB_QD = LDC_SB_W + LDC_ROWS * LDC_WK,
  LDC_SB_ND = LDC_SB_QD + LDC_WK,
  LDC_SB_NE = LDC_SB_ND + 32,
  LDC_SB_TERMS = LDC_SB_NE + 4 * 9,
  LDC_SB_TOTAL = LDC_SB_TERMS + 2 * 4 * LDC_T_N
};
VD constexpr int ldc_fcol(int k) { return k < 6 ? 3 + k : 15 + k; }   // compact column of dF -> column of F
VD constexpr int ldc_terms_at(int slot, int leg) { return LDC_SB_TERMS + LDC_T_N * (4 * slot + leg); }

// What is wrong with the arguments of a call on W windows (null: nothing), without the call's name. Reads offsets[0 .. W], nothing else.
inline const char *leg_dr_cov_check(const vilo_leg_dr_cov_opts &o, int W, const vilo_sample *samples, const int32_t *offsets, const double *state_out,
                                    const double *legs_out, const double *cov_out) {
  return sample_range_check(o.from_frame, o.reserved != 0 ? "reserved must be 0" : nullptr, W, samples, offsets,
                            !state_out ? "state_out is NULL" : (!legs_out ? "legs_out is NULL" : (!cov_out ? "cov_out is NULL" : nullptr)));
}

// Element counts of the call's arrays on W windows with n_rows steps in all (dead_reckon_step_offsets' sum).
struct LegDrCovCounts {
  size_t cov_in, cov, state, legs, pose_traj, leg_traj, rec;
};
inline LegDrCovCounts leg_dr_cov_counts(int W, int32_t n_rows) {
  LegDrCovCounts c;
  const size_t w = W > 0 ? (size_t)W : 0, r = n_rows > 0 ? (size_t)n_rows : 0;
  c.cov_in = (size_t)LDC_IN * LDC_IN * w;
  c.cov = (size_t)LDC_N * LDC_N * w;
  c.state = (size_t)LEGDR_STATE * w;
  c.legs = (size_t)LEGDR_LEGS * w;
  c.pose_traj = (size_t)LDC_POSE * LDC_POSE * r;
  c.leg_traj = (size_t)LDC_LEGCOV * r;
  c.rec = w;
  return c;
}

// E: row i of the 31 coordinates is row ldc_src(i) of the frame block. dp dtheta dv keep their rows, the deps_j rows are the dp rows (a
// leg's world position starts at the frame's position and shares its error), dba dbg drho follow dv in the frame block.
VD constexpr int ldc_src(int i) { return i < LDC_O_EPS ? i : (i < LDC_O_BA ? (i - LDC_O_EPS) % 3 : i - 12); }
// entry (i, j) of Sigma_0 = E cov_in E^T, from the upper triangle of cov_in [19][19]
VD double ldc_sigma0(const double *cov_in, int i, int j) {
  const int a = ldc_src(i), b = ldc_src(j);
  return a <= b ? cov_in[LDC_IN * a + b] : cov_in[LDC_IN * b + a];
}

// What the noise diagonal reads of the configuration (:360-374, :322, :356)
struct LdcNoise {
  double acc_n2, acc_nz2, gyr_n2, acc_w2, gyr_w2, phi_n2, dphi_n2, rho_c_n, rho_nc_n;
};
VD void ldc_noise_const(const vilo_config &cfg, LdcNoise &q) {
  q.acc_n2 = cfg.acc_n * cfg.acc_n; q.acc_nz2 = cfg.acc_n_z * cfg.acc_n_z; q.gyr_n2 = cfg.gyr_n * cfg.gyr_n;
  q.acc_w2 = cfg.acc_w * cfg.acc_w; q.gyr_w2 = cfg.gyr_w * cfg.gyr_w;
  q.phi_n2 = cfg.phi_n * cfg.phi_n; q.dphi_n2 = cfg.dphi_n * cfg.dphi_n;
  q.rho_c_n = cfg.rho_c_n; q.rho_nc_n = cfg.rho_nc_n;
}
// qd[24]: (acc_n, acc_n, acc_n_z)^2, gyr_n^2 (3), those six again, phi_n^2 (6), dphi_n^2 (6)
VD void ldc_dense_noise(const LdcNoise &q, double *qd) {
  for (int e = 0; e < 2; ++e) {
    qd[6 * e] = qd[6 * e + 1] = q.acc_n2; qd[6 * e + 2] = q.acc_nz2;
    qd[6 * e + 3] = qd[6 * e + 4] = qd[6 * e + 5] = q.gyr_n2;
  }
  for (int k = 0; k < 6; ++k) { qd[LDC_W_PHI0 + k] = q.phi_n2; qd[LDC_W_DPHI0 + k] = q.dphi_n2; }
}
// The three uncertainties and the rho_uncertainty of a leg in a step (:290-322, :354-358): flag, variance and lo_v of the step, delta_v
// BEFORE it; all_air: the four flags sum to less than 1e-6. Not squared: they are variances as they stand.
VD void ldc_leg_uncertainty(const LegDrConst &c, const LdcNoise &q, double flag, double ff_var, const v3 &lo_v, const v3 &dv_before, bool all_air,
                            double *unc /* 3 */, double &rho_unc) {
  if (c.contact_sensor_type == 2) {
    const double n1 = c.v_n_max * (1 - flag) + c.v_n_min, n2 = c.term2 * ff_var;
    const v3 tmp = lo_v - dv_before;
    unc[0] = (n1 + n2) + c.term3 * (tmp.x * tmp.x);
    unc[1] = (n1 + n2) + c.term3 * (tmp.y * tmp.y);
    unc[2] = (n1 + n2) + c.term3 * (tmp.z * tmp.z);
  } else {
    unc[0] = unc[1] = c.v_n_max * (1 - flag) + flag * c.v_n_min_xy;
    unc[2] = c.v_n_max * (1 - flag) + flag * c.v_n_min_z;
  }
  rho_unc = q.rho_c_n * flag + q.rho_nc_n;
  if (all_air) {
    rho_unc = q.rho_nc_n;
    unc[0] = unc[1] = unc[2] = 10e10;
  }
}
// ne and nd of leg j: V's blocks at ILNO_V1 + 3 j (:456: -dt I in frame f's body frame, -dt R_f in the world) and ILNO_NRHO (:462-465)
VD void ldc_leg_noise(const m3 &Rf, double dt, const double *unc, double rho_unc, int j, double *sb) {
  double *nd = sb + LDC_SB_ND, *ne = sb + LDC_SB_NE + 9 * j;
  const double d0 = dt * (unc[0] * dt), d1 = dt * (unc[1] * dt), d2 = dt * (unc[2] * dt);
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) ne[3 * a + b] = (Rf.a[3 * a] * d0) * Rf.a[3 * b] + (Rf.a[3 * a + 1] * d1) * Rf.a[3 * b + 1] + (Rf.a[3 * a + 2] * d2) * Rf.a[3 * b + 2];
  nd[LDC_O_RHO + j] = dt * (rho_unc * dt);
}

// terms[LDC_T_N] of a sample and leg (:235-243, :262-286 before the rotations): v is the nominal step's own (legdr_leg_velocity)
VD void ldc_sample_terms(const LegDrConst &c, const v3 &gyr, const double *leg /* phi dphi c */, double rho, const double *rf, const v3 &v, double *t) {
  LegKin k;
  leg_kin_full(leg, rho, rf, k);
  const v3 dphi = ld3(leg + 3);
  const m3 Rw = skew(gyr - c.bg);
  // (dphi^T kron I) dJ/drho = dJ_drho dphi; (dphi^T kron I) dJ/dq = [dJ_0 dphi, dJ_1 dphi, dJ_2 dphi]
  const v3 g0 = c.R_br * (k.dJ_drho * dphi) + Rw * (c.R_br * k.df_drho);
  const v3 k0 = k.dJ[0] * dphi, k1 = k.dJ[1] * dphi, k2 = k.dJ[2] * dphi;
  m3 K;
  K.a[0] = k0.x; K.a[3] = k0.y; K.a[6] = k0.z;
  K.a[1] = k1.x; K.a[4] = k1.y; K.a[7] = k1.z;
  K.a[2] = k2.x; K.a[5] = k2.y; K.a[8] = k2.z;
  const m3 h0 = c.R_br * K + Rw * c.R_br * k.J, BJ = c.R_br * k.J;
  st3(t + LDC_T_V, v);
  st3(t + LDC_T_P, c.p_br + c.R_br * k.f);
  for (int e = 0; e < 9; ++e) { t[LDC_T_H + e] = h0.a[e]; t[LDC_T_J + e] = BJ.a[e]; }
  st3(t + LDC_T_G, g0);
}

VD void ldc_put33(double *M, int ld, int r0, int c0, const m3 &A) {
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b) M[(r0 + a) * ld + c0 + b] = A.a[3 * a + b];
}
// kappa_7 = I - [w]x dt (:392)
VD m3 ldc_kappa7(const v3 &w, double dt) {
  m3 K;
  K.a[0] = 1.0; K.a[1] = w.z * dt; K.a[2] = -(w.y * dt);
  K.a[3] = -(w.z * dt); K.a[4] = 1.0; K.a[5] = w.x * dt;
  K.a[6] = w.y * dt; K.a[7] = -(w.x * dt); K.a[8] = 1.0;
  return K;
}

// Rows dp dtheta dv of dF and W, and nd of dba dbg (:397-413, :434-445, :459-460). R0 = R_f R(delta_q) before the step, R1 =
// R_f R(result_delta_q), a0 = acc_0 - Ba, a1 = acc_1 - Ba, K = kappa_7. The entries that are zero in every step are never written.
VD void ldc_imu_rows(const m3 &R0, const m3 &R1, const m3 &K, const v3 &a0, const v3 &a1, double dt, const LdcNoise &q, double *sb) {
  double *dF = sb + LDC_SB_DF, *W = sb + LDC_SB_W, *nd = sb + LDC_SB_ND;
  const double a = 0.25 * dt * dt, h = 0.5 * dt;
  const m3 C = R1 * skew(a1), AB = R0 * skew(a0) + C * K, S = R0 + R1;
  ldc_put33(dF, LDC_FK, LDC_O_P, LDC_K_R, AB * (-a));
  ldc_put33(dF, LDC_FK, LDC_O_P, LDC_K_V, m3_eye() * dt);
  ldc_put33(dF, LDC_FK, LDC_O_P, LDC_K_BA, S * (-a));
  ldc_put33(dF, LDC_FK, LDC_O_P, LDC_K_BG, C * (a * dt));
  ldc_put33(dF, LDC_FK, LDC_O_R, LDC_K_R, K - m3_eye());
  ldc_put33(dF, LDC_FK, LDC_O_R, LDC_K_BG, m3_eye() * (-dt));
  ldc_put33(dF, LDC_FK, LDC_O_V, LDC_K_R, AB * (-h));
  ldc_put33(dF, LDC_FK, LDC_O_V, LDC_K_BA, S * (-h));
  ldc_put33(dF, LDC_FK, LDC_O_V, LDC_K_BG, C * (h * dt));
  const m3 Cp = C * (-(a * h)), Cv = C * (-(h * h));
  ldc_put33(W, LDC_WK, LDC_O_P, LDC_W_A0, R0 * a); ldc_put33(W, LDC_WK, LDC_O_P, LDC_W_G0, Cp);
  ldc_put33(W, LDC_WK, LDC_O_P, LDC_W_A1, R1 * a); ldc_put33(W, LDC_WK, LDC_O_P, LDC_W_G1, Cp);
  ldc_put33(W, LDC_WK, LDC_O_R, LDC_W_G0, m3_eye() * h); ldc_put33(W, LDC_WK, LDC_O_R, LDC_W_G1, m3_eye() * h);
  ldc_put33(W, LDC_WK, LDC_O_V, LDC_W_A0, R0 * h); ldc_put33(W, LDC_WK, LDC_O_V, LDC_W_G0, Cv);
  ldc_put33(W, LDC_WK, LDC_O_V, LDC_W_A1, R1 * h); ldc_put33(W, LDC_WK, LDC_O_V, LDC_W_G1, Cv);
  for (int k = 0; k < 3; ++k) { nd[LDC_O_BA + k] = dt * (q.acc_w2 * dt); nd[LDC_O_BG + k] = dt * (q.gyr_w2 * dt); }
}
// Rows deps_j of dF and W (:416-424, :448-457) from the terms of the step's two samples, t0 the earlier one
VD void ldc_leg_rows(const m3 &R0, const m3 &R1, const m3 &K, double dt, const double *t0, const double *t1, int j, double *sb) {
  double *dF = sb + LDC_SB_DF, *W = sb + LDC_SB_W;
  const double h = 0.5 * dt;
  const int r = LDC_O_EPS + 3 * j;
  const m3 S0 = R0 * skew(ld3(t0 + LDC_T_V)), S1 = R1 * skew(ld3(t1 + LDC_T_V));
  const m3 P0 = R0 * skew(ld3(t0 + LDC_T_P)), P1 = R1 * skew(ld3(t1 + LDC_T_P));
  ldc_put33(dF, LDC_FK, r, LDC_K_R, (S0 + S1 * K) * (-h));
  ldc_put33(dF, LDC_FK, r, LDC_K_BG, S1 * (h * dt) - (P0 + P1) * h);
  // g_i = -(R0 g0_i), g_ip1 = -(R1 g0_ip1); F(eps_j, rho_j) = dt / 2 (g_i + g_ip1)
  const v3 g = (-(R0 * ld3(t0 + LDC_T_G)) + -(R1 * ld3(t1 + LDC_T_G))) * h;
  dF[(r + 0) * LDC_FK + LDC_K_RHO + j] = g.x; dF[(r + 1) * LDC_FK + LDC_K_RHO + j] = g.y; dF[(r + 2) * LDC_FK + LDC_K_RHO + j] = g.z;
  const m3 Sq = S1 * (-(h * h));
  ldc_put33(W, LDC_WK, r, LDC_W_G0, Sq + P0 * h);
  ldc_put33(W, LDC_WK, r, LDC_W_G1, Sq + P1 * h);
  ldc_put33(W, LDC_WK, r, LDC_W_PHI0, (R0 * ld_m3_rowmajor(t0 + LDC_T_H)) * (-h));
  ldc_put33(W, LDC_WK, r, LDC_W_PHI1, (R1 * ld_m3_rowmajor(t1 + LDC_T_H)) * (-h));
  ldc_put33(W, LDC_WK, r, LDC_W_DPHI0, (R0 * ld_m3_rowmajor(t0 + LDC_T_J)) * (-h));
  ldc_put33(W, LDC_WK, r, LDC_W_DPHI1, (R1 * ld_m3_rowmajor(t1 + LDC_T_J)) * (-h));
}

// Is entry (row i, compact column k) of dF / of W ever written
VD constexpr bool ldc_f_used(int i, int k) {
  return i < LDC_O_R ? k < LDC_K_RHO : i < LDC_O_V ? (k < LDC_K_V || (k >= LDC_K_BG && k < LDC_K_RHO))
       : i < LDC_O_EPS ? (k < LDC_K_V || (k >= LDC_K_BA && k < LDC_K_RHO))
                       : (k < LDC_K_V || (k >= LDC_K_BG && k < LDC_K_RHO) || k == LDC_K_RHO + (i - LDC_O_EPS) / 3);
}
VD constexpr bool ldc_w_used(int i, int k) {
  return (i < LDC_O_R || (i >= LDC_O_V && i < LDC_O_EPS)) ? k < LDC_W_PHI0
       : i < LDC_O_V ? ((k >= LDC_W_G0 && k < LDC_W_A1) || (k >= LDC_W_G1 && k < LDC_W_PHI0))
                     : ((k >= LDC_W_G0 && k < LDC_W_A1) || k >= LDC_W_G1);
}
// c <- F c for a column c[31] of Sigma
VD void ldc_f_times(const double *sb, double *c) {
  const double *dF = sb + LDC_SB_DF;
  double ck[LDC_FK];
  LDC_UNROLL
  for (int k = 0; k < LDC_FK; ++k) ck[k] = c[ldc_fcol(k)];
  LDC_UNROLL
  for (int i = 0; i < LDC_ROWS; ++i) {
    double acc = c[i];
    LDC_UNROLL
    for (int k = 0; k < LDC_FK; ++k)
      if (ldc_f_used(i, k)) acc = fma(dF[LDC_FK * i + k], ck[k], acc);
    c[i] = acc;
    LDC_ROW_DONE
  }
}
// c += V Q V^T e_j for column j (31: the padding column, nothing)
VD void ldc_add_noise(const double *sb, int j, double *c) {
  const double *W = sb + LDC_SB_W, *qd = sb + LDC_SB_QD, *nd = sb + LDC_SB_ND, *ne = sb + LDC_SB_NE;
  if (j < LDC_ROWS) {
    double wq[LDC_WK];
    LDC_UNROLL
    for (int k = 0; k < LDC_WK; ++k) wq[k] = W[LDC_WK * j + k] * qd[k];
    LDC_UNROLL
    for (int i = 0; i < LDC_ROWS; ++i) {
      double acc = c[i];
      LDC_UNROLL
      for (int k = 0; k < LDC_WK; ++k)
        if (ldc_w_used(i, k)) acc = fma(W[LDC_WK * i + k], wq[k], acc);
      c[i] = acc;
      LDC_ROW_DONE
    }
  }
  // (a select per compile-time row, not c[j]: the kernel's j differs between lanes and c lives in registers)
  const bool eps = j >= LDC_O_EPS && j < LDC_O_BA;
  const int l = eps ? (j - LDC_O_EPS) / 3 : 0, jj = eps ? (j - LDC_O_EPS) - 3 * l : 0;
  const double e0 = eps ? ne[9 * l + jj] : 0.0, e1 = eps ? ne[9 * l + 3 + jj] : 0.0, e2 = eps ? ne[9 * l + 6 + jj] : 0.0;
  LDC_UNROLL
  for (int i = LDC_O_EPS; i < LDC_O_BA; ++i) {
    const int a = (i - LDC_O_EPS) % 3;
    c[i] += eps && (i - LDC_O_EPS) / 3 == l ? (a == 0 ? e0 : (a == 1 ? e1 : e2)) : 0.0;
  }
  const double nj = j >= LDC_O_BA && j < LDC_N ? nd[j] : 0.0;
  LDC_UNROLL
  for (int i = LDC_O_BA; i < LDC_N; ++i) c[i] += i == j ? nj : 0.0;
}

// The step block before the first step: zeros, and the constant variances
VD void ldc_block_start(const LdcNoise &q, double *sb) {
  for (int i = 0; i < LDC_SB_TOTAL; ++i) sb[i] = 0.0;
  ldc_dense_noise(q, sb + LDC_SB_QD);
}

// The CPU path: one window whose frame f exists, through rows[n][LEGDR_ROW]. pose: frame f's 7, sb9: its 9 (V, Ba, Bg), lb: its 4;
// cov_in: null or [19][19]. cov [31][31]; pose_traj: null or [n - 1][6][6]; leg_traj: null or [n - 1][4][3][3]. Returns VILO_DR_OK or
// VILO_DR_NUMERIC (then every row is zeros).
inline int leg_dr_cov_window(const vilo_config &cfg, const double *pose, const double *sb9, const double *lb, const double *rows, int n, const double *cov_in,
                             double *state, double *legs, double *cov, double *pose_traj, double *leg_traj) {
  const int n_steps = n > 1 ? n - 1 : 0;
  const LegDrAllLegs x;
  LegDrWalk<4> w;
  bool finite = legdr_window_start(cfg, pose, sb9, lb, n_steps ? rows : nullptr, x, w);
  const LegDrConst &c = w.c;
  LegDrState<4> &s = w.s;
  LegDrStep<4> &o = w.o;
  double S[LDC_N][LDC_N];   // S[j]: column j of Sigma
  for (int j = 0; j < LDC_N; ++j)
    for (int i = 0; i < LDC_N; ++i) {
      S[j][i] = cov_in ? ldc_sigma0(cov_in, i, j) : 0.0;
      finite = finite && legdr_finite(S[j][i]);
    }
  LdcNoise q;
  ldc_noise_const(cfg, q);
  double sb[LDC_SB_TOTAL];
  ldc_block_start(q, sb);
  if (n_steps)
    for (int l = 0; l < 4; ++l) ldc_sample_terms(c, s.gyr0, w.lg[l], s.rho[l], s.rf[l], s.v0[l], sb + ldc_terms_at(0, l));
  for (int i = 1; i < n; ++i) {
    finite = legdr_next_row(rows + (size_t)LEGDR_ROW * i, x, w) && finite;
    const quat dq0 = s.dq;
    const v3 dv0 = s.dv, acc0 = s.acc0, gyr0 = s.gyr0;
    legdr_step(c, s, w.sh, w.lg, x, o);
    const double dt = w.sh[0];
    const m3 R0 = w.wf.R0 * qR(dq0), R1 = w.wf.R0 * qR(o.rq);
    const m3 K = ldc_kappa7(0.5 * (gyr0 + s.gyr0) - c.bg, dt);
    const bool all_air = o.flag[0] + o.flag[1] + o.flag[2] + o.flag[3] < 1e-6;
    const int e0 = (i - 1) & 1, e1 = i & 1;
    for (int l = 0; l < 4; ++l) {
      ldc_sample_terms(c, s.gyr0, w.lg[l], s.rho[l], s.rf[l], s.v0[l], sb + ldc_terms_at(e1, l));
      double unc[3], rho_unc;
      ldc_leg_uncertainty(c, q, o.flag[l], s.ff_var[l], o.lo_v[l], dv0, all_air, unc, rho_unc);
      ldc_leg_noise(w.wf.R0, dt, unc, rho_unc, l, sb);
      ldc_leg_rows(R0, R1, K, dt, sb + ldc_terms_at(e0, l), sb + ldc_terms_at(e1, l), l, sb);
    }
    ldc_imu_rows(R0, R1, K, acc0 - c.ba, s.acc0 - c.ba, dt, q, sb);
    for (int j = 0; j < LDC_N; ++j) ldc_f_times(sb, S[j]);
    for (int j = 0; j < LDC_N; ++j)
      for (int k = 0; k < j; ++k) { const double t = S[j][k]; S[j][k] = S[k][j]; S[k][j] = t; }
    for (int j = 0; j < LDC_N; ++j) {
      ldc_f_times(sb, S[j]);
      ldc_add_noise(sb, j, S[j]);
    }
    if (pose_traj)
      for (int j = 0; j < LDC_POSE; ++j)
        for (int k = 0; k <= j; ++k) {
          double *d = pose_traj + (size_t)(LDC_POSE * LDC_POSE) * (i - 1);
          d[LDC_POSE * k + j] = d[LDC_POSE * j + k] = S[j][k];
        }
    if (leg_traj)
      for (int l = 0; l < 4; ++l)
        for (int j = 0; j < 3; ++j)
          for (int k = 0; k <= j; ++k) {
            double *d = leg_traj + (size_t)LDC_LEGCOV * (i - 1) + 9 * l;
            d[3 * k + j] = d[3 * j + k] = S[LDC_O_EPS + 3 * l + j][LDC_O_EPS + 3 * l + k];
          }
  }
  legdr_state_row(w.wf, s, o.flag, x, state, legs);
  finite = finite && legdr_rows_finite(state, legs, x);
  for (int j = 0; j < LDC_N; ++j)
    for (int k = 0; k <= j; ++k) {
      finite = finite && legdr_finite(S[j][k]);
      cov[LDC_N * k + j] = cov[LDC_N * j + k] = S[j][k];
    }
  if (!finite) {
    legdr_zero_share(x, state, LEGDR_STATE);
    legdr_zero_share(x, legs, LEGDR_LEGS);
    for (int i = 0; i < LDC_N * LDC_N; ++i) cov[i] = 0.0;
    if (pose_traj)
      for (size_t i = 0; i < (size_t)(LDC_POSE * LDC_POSE) * n_steps; ++i) pose_traj[i] = 0.0;
    if (leg_traj)
      for (size_t i = 0; i < (size_t)LDC_LEGCOV * n_steps; ++i) leg_traj[i] = 0.0;
    return VILO_DR_NUMERIC;
  }
  return VILO_DR_OK;
}

}  // namespace vilo
