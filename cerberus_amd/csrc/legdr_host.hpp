// Leg-odometry dead reckoning of a frame (vilo_batch_leg_dead_reckon, include/vilo_gpu.h; kernels_legdr.hip): the part that needs no
// device. The argument checks, the packing of the samples, the row layouts, and the step itself: legdr_step is the nominal-state part of
// IMULegIntegrationBase::midPointIntegration (imu_leg_integration_base.cpp:152-158, :181-257, :290-351) followed by propagate()'s carry
// (:121-135), literally and in that order of operations, without the Jacobian, covariance, g / h and noise_diag work. It is one
// __host__ __device__ function over plain arrays; what differs between its two callers is how many legs a caller owns and how the four
// legs' values meet (the policy X):
//   LegDrAllLegs   a CPU thread owns the four legs of a window (leg_dead_reckon_window below; tests/host_check/leg_dr_check.cpp)
//   the kernel's   a lane owns one leg, the four lanes of a quad own a window, the values meet by DPP (kernels_legdr.hip)
// Either way the sums over the legs run in the fixed order j = 0, 1, 2, 3, so the two callers round alike.
// The all-feet-in-the-air case (:354-358) only overwrites uncertainties that go to noise_diag, after the weights were taken: it changes
// nothing here. delta_p (:157) reaches no output of the call and is not carried. foot_contact_flag is the reference's Vector4i: under
// contact_sensor_type 2 the logistic value is truncated to 0 or 1 (:215), as vilo_preintegrate does.
// Kinematics: vilo_math.hpp's leg_fk_jac. Contact-force filter: the 36 doubles of preint_blocks.hpp's O_FF layout (min, max, variance:
// 4 each; window 4 x 5; index 4), a leg's nine of them per owned leg; legdr_ff_export writes them back in that layout.
// HIP-free when compiled by a host compiler.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "deadreckon_host.hpp"
#include "preint_blocks.hpp"
#include "vilo_math.hpp"

namespace vilo {

#define LEGDR_STATE 32   // doubles of a state_out row (LS_*)
#define LEGDR_LEGS 12    // doubles of a legs_out row: the four legs' world positions
#define LEGDR_TRAJ 48    // doubles of a trajectory row (LT_*)
#define LEGDR_ROW 35     // doubles of a packed sample: dt acc gyr (7), then per leg phi (3) dphi (3) c (1)
#define LEGDR_ROW_SHARED 7
#define LEGDR_ROW_LEG 7
constexpr int LEGDR_FF_N = pb::O_COEF - pb::O_FF;   // the filter state of an IMULegIntegrationBase object
static_assert(LEGDR_FF_N == 36, "preint_blocks.hpp: O_FF holds min, max, variance (4 each), window (4 x 5), index (4)");
constexpr int LEGDR_FF_WIN = 5;   // FOOT_VAR_WINDOW_SIZE
VD constexpr int ff_min_at(int j) { return j; }
VD constexpr int ff_max_at(int j) { return 4 + j; }
VD constexpr int ff_var_at(int j) { return 8 + j; }
VD constexpr int ff_win_at(int j, int k) { return 12 + LEGDR_FF_WIN * j + k; }
VD constexpr int ff_idx_at(int j) { return 32 + j; }

enum { LS_SUM_DT = 0, LS_DQ = 1, LS_DV = 5, LS_EPS = 8, LS_SUM_EPS = 20, LS_POS = 23, LS_FLAG = 26, LS_PAD = 30 };
enum { LT_SUM_DT = 0, LT_POS = 1, LT_VEL = 4, LT_FLAG = 7, LT_LOV = 11, LT_W = 23, LT_FOOT = 35, LT_PAD = 47 };

// What is wrong with the arguments of a call on W windows (null: nothing), without the call's name. Reads offsets[0 .. W], nothing else.
inline const char *leg_dead_reckon_check(const vilo_leg_dead_reckon_opts &o, int W, const vilo_sample *samples, const int32_t *offsets,
                                         const double *state_out, const double *legs_out) {
  return sample_range_check(o.from_frame, o.reserved != 0 ? "reserved must be 0" : nullptr, W, samples, offsets,
                            !state_out ? "state_out is NULL" : (!legs_out ? "legs_out is NULL" : nullptr));
}

// out[n][LEGDR_ROW]: what a quad of lanes loads in one step lies together: dt acc gyr, then leg j's phi dphi c at 7 + 7 j
inline void leg_dead_reckon_pack(const vilo_sample *samples, size_t n, double *out) {
  for (size_t i = 0; i < n; ++i) {
    double *r = out + LEGDR_ROW * i;
    const vilo_sample &s = samples[i];
    r[0] = s.dt;
    for (int k = 0; k < 3; ++k) { r[1 + k] = s.acc[k]; r[4 + k] = s.gyr[k]; }
    for (int j = 0; j < 4; ++j) {
      double *l = r + LEGDR_ROW_SHARED + LEGDR_ROW_LEG * j;
      for (int k = 0; k < 3; ++k) { l[k] = s.phi[3 * j + k]; l[3 + k] = s.dphi[3 * j + k]; }
      l[6] = s.c[j];
    }
  }
}

VD bool legdr_finite(double x) { return fabs(x) <= 1.79769313486231570815e308; }   // (false for a NaN)

// What a range of steps reads of the configuration and of frame f: constant over the range
struct LegDrConst {
  int contact_sensor_type;
  double thres_ratio, steep, v_n_max, v_n_min_xy, v_n_min_z, v_n_min, term2, term3;
  m3 R_br;
  v3 p_br, ba, bg;
};
VD void legdr_const(const vilo_config &cfg, const double *ba, const double *bg, LegDrConst &c) {
  c.contact_sensor_type = cfg.contact_sensor_type;
  c.thres_ratio = cfg.v_n_force_thres_ratio; c.steep = cfg.v_n_term1_steep; c.v_n_max = cfg.v_n_max;
  c.v_n_min_xy = cfg.v_n_min_xy; c.v_n_min_z = cfg.v_n_min_z; c.v_n_min = cfg.v_n_min;
  c.term2 = cfg.v_n_term2_var_rescale; c.term3 = cfg.v_n_term3_distance_rescale;
  c.R_br = ld_m3_rowmajor(cfg.R_br);
  c.p_br = ld3(cfg.p_br); c.ba = ld3(ba); c.bg = ld3(bg);
}

// The integration object between two steps, N legs of it: the public state, the previous sample and the contact-force filter
template <int N> struct LegDrState {
  double sum_dt;
  quat dq;
  v3 dv, sum_eps;
  v3 acc0, gyr0;
  v3 eps[N], v0[N];          // delta_epsilon; the body-frame velocity v_i of the previous sample (:242, which is :243 of the step before)
  double c0[N];
  double rho[N], rf[N][4];   // linearized_rho and rho_fix_list of the leg
  double ff_min[N], ff_max[N], ff_var[N], ff_win[N][LEGDR_FF_WIN];
  int ff_idx[N];
};
// What a step leaves beside the state: a trajectory row's values in the body frame of frame f
template <int N> struct LegDrStep {
  quat rq;                   // result_delta_q (:154), un-normalised
  v3 vel;                    // sum_j w_j o lo_v_j / sum_j w_j
  double flag[N];
  v3 lo_v[N], w[N], foot[N]; // :255; :335-340; p_br + R_br fk(phi_1)
};

struct LegDrAllLegs {
  static constexpr int N = 4;
  VD int leg(int l) const { return l; }
  VD bool first() const { return true; }
  VD void gather(const double (&mine)[N], double (&all)[4]) const { for (int j = 0; j < 4; ++j) all[j] = mine[j]; }
  VD bool all_of(bool v) const { return v; }
};

// v of a sample and leg (:242 / :243): -R_br J dphi - [gyr - bg]x (p_br + R_br fk), and p_br + R_br fk
VD v3 legdr_leg_velocity(const LegDrConst &c, const v3 &gyr, const double *leg /* phi dphi c */, double rho, const double *rf, v3 &foot) {
  v3 f;
  m3 J;
  leg_fk_jac(leg, rho, rf, f, J);
  foot = c.p_br + c.R_br * f;
  return ((-c.R_br) * J) * ld3(leg + 3) - skew(gyr - c.bg) * foot;
}

// The constructor (:7-47) at frame f's biases with the first sample of the range as (acc_0, gyr_0, phi_0, dphi_0, c_0)
template <class X>
VD void legdr_start(const LegDrConst &c, const vilo_config &cfg, const double *leg_bias /* frame f's 4 */, const double *sh0, const double (*leg0)[LEGDR_ROW_LEG],
                    const X &x, LegDrState<X::N> &s) {
  s.sum_dt = 0.0;
  s.dq = mkq(1, 0, 0, 0);
  s.dv = mk3(0, 0, 0); s.sum_eps = mk3(0, 0, 0);
  s.acc0 = sh0 ? ld3(sh0 + 1) : mk3(0, 0, 0);
  s.gyr0 = sh0 ? ld3(sh0 + 4) : mk3(0, 0, 0);
  for (int l = 0; l < X::N; ++l) {
    const int j = x.leg(l);
    s.eps[l] = mk3(0, 0, 0);
    s.rho[l] = leg_bias[j];
    for (int k = 0; k < 4; ++k) s.rf[l][k] = cfg.rho_fix[j][k];
    s.ff_min[l] = s.ff_max[l] = s.ff_var[l] = 0.0;
    for (int k = 0; k < LEGDR_FF_WIN; ++k) s.ff_win[l][k] = 0.0;
    s.ff_idx[l] = 0;
    v3 foot;
    s.v0[l] = sh0 ? legdr_leg_velocity(c, s.gyr0, leg0[l], s.rho[l], s.rf[l], foot) : mk3(0, 0, 0);
    s.c0[l] = sh0 ? leg0[l][6] : 0.0;
  }
}

// One push_back: sh1 = dt acc gyr of the sample, leg1[l] = phi dphi c of owned leg l
template <class X>
VD void legdr_step(const LegDrConst &c, LegDrState<X::N> &s, const double *sh1, const double (*leg1)[LEGDR_ROW_LEG], const X &x, LegDrStep<X::N> &o) {
  constexpr int N = X::N;
  const double dt = sh1[0];
  const v3 acc1 = ld3(sh1 + 1), gyr1 = ld3(sh1 + 4);
  // :152-158
  const v3 un_acc_0 = qrot(s.dq, s.acc0 - c.ba);
  const v3 un_gyr = 0.5 * (s.gyr0 + gyr1) - c.bg;
  const quat rq = qmul(s.dq, mkq(1, un_gyr.x * dt / 2, un_gyr.y * dt / 2, un_gyr.z * dt / 2));
  const v3 un_acc_1 = qrot(rq, acc1 - c.ba);
  const v3 un_acc = 0.5 * (un_acc_0 + un_acc_1);
  const v3 r_dv = s.dv + un_acc * dt;
  o.rq = rq;
  double wl[3][N], wv[3][N];   // the owned legs' weights and weighted velocities, by component
  for (int l = 0; l < N; ++l) {
    const double c1 = leg1[l][6];
    // :183-229
    double flag;
    if (c.contact_sensor_type == 2) {
      const double force_mag = 0.5 * (s.c0[l] + c1);
      double fmn = s.ff_min[l], fmx = s.ff_max[l];
      if (force_mag < fmn) fmn = 0.9 * fmn + 0.1 * force_mag;
      if (force_mag > fmx) fmx = 0.9 * fmx + 0.1 * force_mag;
      fmn *= 0.9991;
      fmx *= 0.997;
      const double thr = fmn + c.thres_ratio * (fmx - fmn);
      // Vector4i foot_contact_flag: the value in [0, 1] is truncated, 1 only where it rounds to 1
      flag = 1.0 / (1 + exp(-c.steep * (force_mag - thr))) >= 1.0 ? 1.0 : 0.0;
      const int idx = (s.ff_idx[l] + 1) % LEGDR_FF_WIN;
      double mean = 0.0;
      for (int k = 0; k < LEGDR_FF_WIN; ++k) {   // (no register array is indexed by a run-time value)
        if (k == idx) s.ff_win[l][k] = force_mag;
        mean += s.ff_win[l][k];
      }
      mean /= LEGDR_FF_WIN;
      double ss = 0.0;
      for (int k = 0; k < LEGDR_FF_WIN; ++k) ss += (s.ff_win[l][k] - mean) * (s.ff_win[l][k] - mean);
      s.ff_min[l] = fmn; s.ff_max[l] = fmx; s.ff_var[l] = ss / (LEGDR_FF_WIN - 1); s.ff_idx[l] = idx;
    } else {
      flag = c1 >= 0.5 ? 1.0 : 0.0;
    }
    // :232-257
    const v3 v1 = legdr_leg_velocity(c, gyr1, leg1[l], s.rho[l], s.rf[l], o.foot[l]);
    const v3 lo_v = 0.5 * (qrot(s.dq, s.v0[l]) + qrot(rq, v1));
    s.eps[l] = s.eps[l] + lo_v * dt;
    // :290-317
    double unc[3];
    if (c.contact_sensor_type == 2) {
      const double n1 = c.v_n_max * (1 - flag) + c.v_n_min, n2 = c.term2 * s.ff_var[l];
      const v3 tmp = lo_v - s.dv;
      unc[0] = (n1 + n2) + c.term3 * (tmp.x * tmp.x);
      unc[1] = (n1 + n2) + c.term3 * (tmp.y * tmp.y);
      unc[2] = (n1 + n2) + c.term3 * (tmp.z * tmp.z);
    } else {
      unc[0] = unc[1] = c.v_n_max * (1 - flag) + flag * c.v_n_min_xy;
      unc[2] = c.v_n_max * (1 - flag) + flag * c.v_n_min_z;
    }
    // :335-340
    const double K = c.v_n_max + c.term2 + c.term3;
    for (int k = 0; k < 3; ++k) {
      double wk = K / unc[k];
      if (wk < 0.001) wk = 0.001;
      wl[k][l] = wk;
      wv[k][l] = wk * at(lo_v, k);
    }
    o.flag[l] = flag;
    o.lo_v[l] = lo_v;
    o.w[l] = mk3(wl[0][l], wl[1][l], wl[2][l]);
    s.v0[l] = v1;
    s.c0[l] = c1;
  }
  // :341-351, the four legs in the order j = 0 .. 3
  double avg[3], vel[3];
  for (int k = 0; k < 3; ++k) {
    double w4[4], wv4[4];
    x.gather(wl[k], w4);
    x.gather(wv[k], wv4);
    double a = 0.0, cnt = 0.0, v = 0.0;
    for (int j = 0; j < 4; ++j) { a += wv4[j] * dt; cnt += w4[j]; v += wv4[j]; }
    avg[k] = a / cnt;
    vel[k] = v / cnt;
  }
  s.sum_eps = s.sum_eps + mk3(avg[0], avg[1], avg[2]);
  o.vel = mk3(vel[0], vel[1], vel[2]);
  // propagate(), :121-135
  s.dv = r_dv;
  s.dq = qnormalized(rq);
  s.sum_dt += dt;
  s.acc0 = acc1; s.gyr0 = gyr1;
}

// The world frame of the outputs: R0 = R(q_f / |q_f|), P0
struct LegDrWorld {
  m3 R0;
  v3 P0;
};
// state_out[LEGDR_STATE] and legs_out[LEGDR_LEGS] of a window; every caller writes its legs' entries, the first one the shared ones
template <class X>
VD void legdr_state_row(const LegDrWorld &wf, const LegDrState<X::N> &s, const double (&flag)[X::N], const X &x, double *state, double *legs) {
  if (x.first()) {
    state[LS_SUM_DT] = s.sum_dt;
    state[LS_DQ] = s.dq.x; state[LS_DQ + 1] = s.dq.y; state[LS_DQ + 2] = s.dq.z; state[LS_DQ + 3] = s.dq.w;
    st3(state + LS_DV, s.dv);
    st3(state + LS_SUM_EPS, s.sum_eps);
    st3(state + LS_POS, wf.P0 + wf.R0 * s.sum_eps);
    state[LS_PAD] = state[LS_PAD + 1] = 0.0;
  }
  for (int l = 0; l < X::N; ++l) {
    const int j = x.leg(l);
    st3(state + LS_EPS + 3 * j, s.eps[l]);
    state[LS_FLAG + j] = flag[l];
    st3(legs + 3 * j, wf.P0 + wf.R0 * s.eps[l]);
  }
}
// a trajectory row [LEGDR_TRAJ] after a step
template <class X>
VD void legdr_traj_row(const LegDrWorld &wf, const LegDrState<X::N> &s, const LegDrStep<X::N> &o, const X &x, double *row) {
  const v3 pos = wf.P0 + wf.R0 * s.sum_eps;
  if (x.first()) {
    row[LT_SUM_DT] = s.sum_dt;
    st3(row + LT_POS, pos);
    st3(row + LT_VEL, wf.R0 * o.vel);
    row[LT_PAD] = 0.0;
  }
  for (int l = 0; l < X::N; ++l) {
    const int j = x.leg(l);
    row[LT_FLAG + j] = o.flag[l];
    st3(row + LT_LOV + 3 * j, wf.R0 * o.lo_v[l]);
    st3(row + LT_W + 3 * j, o.w[l]);
    st3(row + LT_FOOT + 3 * j, pos + wf.R0 * qrot(o.rq, o.foot[l]));
  }
}
// are the entries this caller wrote of state_out and legs_out finite
template <class X>
VD bool legdr_rows_finite(const double *state, const double *legs, const X &x) {
  bool ok = true;
  if (x.first()) {
    for (int i = 0; i < LS_EPS; ++i) ok = ok && legdr_finite(state[i]);
    for (int i = LS_SUM_EPS; i < LS_FLAG; ++i) ok = ok && legdr_finite(state[i]);
  }
  for (int l = 0; l < X::N; ++l)
    for (int i = 0; i < 3; ++i) ok = ok && legdr_finite(state[LS_EPS + 3 * x.leg(l) + i]) && legdr_finite(legs[3 * x.leg(l) + i]);
  return ok;
}

// A caller's walk through a range: what is constant over it, the integration object, the last step's by-products and the row in hand
template <int N> struct LegDrWalk {
  LegDrConst c;
  LegDrWorld wf;
  LegDrState<N> s;
  LegDrStep<N> o;
  double sh[LEGDR_ROW_SHARED], lg[N][LEGDR_ROW_LEG];   // dt acc gyr; phi dphi c of every owned leg
};
// r[LEGDR_ROW] as its caller reads it. from 1: the first sample of a range, whose dt is not read
template <class X>
VD void legdr_load_row(const double *r, int from, const X &x, double *sh, double (*lg)[LEGDR_ROW_LEG]) {
  if (from) sh[0] = 0.0;
  for (int k = from; k < LEGDR_ROW_SHARED; ++k) sh[k] = r[k];
  for (int l = 0; l < X::N; ++l)
    for (int k = 0; k < LEGDR_ROW_LEG; ++k) lg[l][k] = r[LEGDR_ROW_SHARED + LEGDR_ROW_LEG * x.leg(l) + k];
}
template <class X>
VD bool legdr_row_finite(int from, const X &, const double *sh, const double (*lg)[LEGDR_ROW_LEG]) {
  bool ok = true;
  for (int k = from; k < LEGDR_ROW_SHARED; ++k) ok = ok && legdr_finite(sh[k]);
  for (int l = 0; l < X::N; ++l)
    for (int k = 0; k < LEGDR_ROW_LEG; ++k) ok = ok && legdr_finite(lg[l][k]);
  return ok;
}
// the row of the next step into w; returns whether it is finite
template <class X>
VD bool legdr_next_row(const double *r, const X &x, LegDrWalk<X::N> &w) {
  legdr_load_row(r, 0, x, w.sh, w.lg);
  return legdr_row_finite(0, x, w.sh, w.lg);
}
// The start of a walk at a frame (pose: its 7, sb: its 9 (V, Ba, Bg), lb: its 4) with row0, the first sample of the range (null: a range
// without steps). Returns whether what the caller read, of the frame for its legs and of the row, is finite.
template <class X>
VD bool legdr_window_start(const vilo_config &cfg, const double *pose, const double *sb, const double *lb, const double *row0, const X &x, LegDrWalk<X::N> &w) {
  bool finite = true;
  for (int l = 0; l < X::N; ++l) finite = finite && legdr_finite(lb[x.leg(l)]);
  for (int k = 0; k < 7; ++k) finite = finite && legdr_finite(pose[k]);
  for (int k = 3; k < 9; ++k) finite = finite && legdr_finite(sb[k]);
  legdr_const(cfg, sb + 3, sb + 6, w.c);
  w.wf.R0 = qR(qnormalized(ldq_pose(pose)));
  w.wf.P0 = ld3(pose);
  for (int l = 0; l < X::N; ++l) w.o.flag[l] = 0.0;
  if (row0) {
    legdr_load_row(row0, 1, x, w.sh, w.lg);
    finite = finite && legdr_row_finite(1, x, w.sh, w.lg);
    legdr_start(w.c, cfg, lb, w.sh, w.lg, x, w.s);
  } else {
    legdr_start(w.c, cfg, lb, (const double *)nullptr, (const double (*)[LEGDR_ROW_LEG])nullptr, x, w.s);
  }
  return finite;
}
// Zeros in the caller's share of p[n]: the owner of N of the four legs takes every (4 / N)-th entry from its first leg's on
template <class X>
VD void legdr_zero_share(const X &x, double *p, size_t n) {
  for (size_t i = x.leg(0); i < n; i += 4 / X::N) p[i] = 0.0;
}

// the filter of the four legs in the O_FF layout
inline void legdr_ff_export(const LegDrState<4> &s, double *ff /* LEGDR_FF_N */) {
  for (int j = 0; j < 4; ++j) {
    ff[ff_min_at(j)] = s.ff_min[j]; ff[ff_max_at(j)] = s.ff_max[j]; ff[ff_var_at(j)] = s.ff_var[j]; ff[ff_idx_at(j)] = (double)s.ff_idx[j];
    for (int k = 0; k < LEGDR_FF_WIN; ++k) ff[ff_win_at(j, k)] = s.ff_win[j][k];
  }
}

// The CPU path: one window whose frame f exists, through rows[n][LEGDR_ROW]. pose: frame f's 7, sb: its 9 (V, Ba, Bg), lb: its 4.
// traj: null or [max(0, n - 1)][LEGDR_TRAJ]; ff_out: null or [LEGDR_FF_N]. Returns VILO_DR_OK or VILO_DR_NUMERIC (then the rows are zeros).
// Like the kernel, this path (and leg_dr_cov_window) walks on through a non-finite row and zeroes its outputs at the end: legdr_step and
// the ldc_* functions must stay free of double-to-integer conversions and of indices computed from sample values, which a NaN would
// make undefined.
inline int leg_dead_reckon_window(const vilo_config &cfg, const double *pose, const double *sb, const double *lb, const double *rows, int n,
                                  double *state, double *legs, double *traj, double *ff_out) {
  const int n_steps = n > 1 ? n - 1 : 0;
  const LegDrAllLegs x;
  LegDrWalk<4> w;
  bool finite = legdr_window_start(cfg, pose, sb, lb, n_steps ? rows : nullptr, x, w);
  for (int i = 1; i < n; ++i) {
    finite = legdr_next_row(rows + (size_t)LEGDR_ROW * i, x, w) && finite;
    legdr_step(w.c, w.s, w.sh, w.lg, x, w.o);
    if (traj) legdr_traj_row(w.wf, w.s, w.o, x, traj + (size_t)LEGDR_TRAJ * (i - 1));
  }
  legdr_state_row(w.wf, w.s, w.o.flag, x, state, legs);
  finite = finite && legdr_rows_finite(state, legs, x);
  if (ff_out) legdr_ff_export(w.s, ff_out);
  if (!finite) {
    legdr_zero_share(x, state, LEGDR_STATE);
    legdr_zero_share(x, legs, LEGDR_LEGS);
    if (traj) legdr_zero_share(x, traj, (size_t)LEGDR_TRAJ * n_steps);
    if (ff_out)
      for (int i = 0; i < LEGDR_FF_N; ++i) ff_out[i] = 0.0;
    return VILO_DR_NUMERIC;
  }
  return VILO_DR_OK;
}

}  // namespace vilo
