// The stepping of one window by one wave, x [+] alpha * delta, as k_retract (kernels_retract.hip) applies it in place and k_trial_states
// (kernels_trial.hip) writes it into a call's scratch: the same two passes over the same items, so a trial state is bit for bit the state
// vilo_batch_retract leaves. Lanes 0 .. 12 own the 11 pose and 2 extrinsic blocks, a strided pass covers the 144 Euclidean coordinates and
// the landmarks (caller order through lm_perm, the mask in device order).
//
// Rounding. s = alpha * delta and x + s are each rounded once (rt_mul / rt_add: contraction off), so numpy restates them to the bit
// (tests/retract_ref.py); pose_plus runs as a function of its own (rt_pose_plus), so a pose block is bit for bit vilo_pose_plus(x, s).
#pragma once
#include "solver_types.hpp"
#include "vilo_math.hpp"

#define RT_STATE 222                      // vilo_batch_gradient's state_grad row
#define RT_SB 66                          // its speed-bias, leg-bias, extrinsic and td entries
#define RT_LB 165
#define RT_EX 209
#define RT_TD 221
#define RT_EUCLID (99 + 44 + 1)           // Euclidean coordinates of a window: speed-bias, leg bias, td

namespace {

__device__ __forceinline__ double rt_mul(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double rt_add(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}

// vilo::pose_plus as a function of its own, memory to memory, the way k_pose_plus (kernels_eval.hip) runs it. Which of a quaternion
// product's multiplies the compiler fuses into the following addition depends on what surrounds the expression: inlined here on steps that
// are themselves products in registers, it fuses qw * bz instead of qx * by in the z component and the result is an ulp off
// vilo_pose_plus's. Compiled on its own it is instruction for instruction k_pose_plus's arithmetic (tests/test_retract_gpu.py holds the
// bytes). The 13 lanes that call it pass the step and take the result through private memory.
__device__ __noinline__ void rt_pose_plus(const double *x, const double *s, double *out) { vilo::pose_plus(x, s, out); }

// count, max |s| and sum s^2 (hi + lo, TwoSum) of the steps a lane applies
struct StepStats {
  double hi, lo, mx;
  int n, bad;
};
__device__ __forceinline__ void rt_two_sum(double &hi, double &lo, double v, double vlo) {
#pragma clang fp contract(off)
  const double t = hi + v, bb = t - hi, e = (hi - (t - bb)) + (v - bb);
  hi = t;
  lo = (lo + vlo) + e;
}
__device__ __forceinline__ void rt_count(StepStats &st, double s) {
  st.bad |= !isfinite(s);
  st.n += 1;
  st.mx = fmax(st.mx, fabs(s));
  rt_two_sum(st.hi, st.lo, rt_mul(s, s), 0.0);
}

// Euclidean coordinate e < RT_EUCLID of a window: its entry of the state row, of the step row, and whether it is stepped
__device__ __forceinline__ bool rt_euclid(int e, int F, int use_leg, int cmask, int &xo, int &so) {
  if (e < 99) { xo = XO_SB + e; so = RT_SB + e; return e / 9 < F; }
  if (e < 143) { xo = XO_LB + (e - 99); so = RT_LB + (e - 99); return (e - 99) / 4 < F && use_leg && !(cmask & CONST_LB); }
  xo = XO_TD; so = RT_TD;
  return !(cmask & CONST_TD);
}
// pose-type block blk < 13 (11 frames, 2 extrinsics)
__device__ __forceinline__ bool rt_block(int blk, int F, int cmask, int &xo, int &so) {
  if (blk < 11) { xo = XO_POSE + 7 * blk; so = 6 * blk; return blk < F; }
  xo = XO_EX + 7 * (blk - 11); so = RT_EX + 6 * (blk - 11);
  return !(cmask & CONST_EX);
}

// One window's step as its wave sees it. step: the window's row of RT_STATE, or null (zero); lm_step: the window's L entries in caller
// order, or null; mask / perm: the batch's tables (device order, indexed from wm.lm_off).
struct StepView {
  const double *step, *lm_step;
  const unsigned char *mask;
  const int *perm;
  double al;
};

// pass 1: every s = alpha * delta that would be applied, tested, counted and summed per lane; nothing is stored
__device__ __forceinline__ StepStats rt_scan(const WinMeta &wm, const StepView &v, int lane) {
  const int F = wm.n_frames, cmask = wm.const_mask, L = wm.L;
  StepStats st = {0.0, 0.0, 0.0, 0, !isfinite(v.al)};
  int bxo = 0, bso = 0;
  if (lane < 13 && rt_block(lane, F, cmask, bxo, bso))
    for (int c = 0; c < 6; ++c) rt_count(st, rt_mul(v.al, v.step ? v.step[bso + c] : 0.0));
  for (int e = lane; e < RT_EUCLID; e += 64) {
    int xo, so;
    if (rt_euclid(e, F, wm.use_leg, cmask, xo, so)) rt_count(st, rt_mul(v.al, v.step ? v.step[so] : 0.0));
  }
  for (int l = lane; l < L; l += 64) {
    const int gi = wm.lm_off + l;
    if (!(v.mask && v.mask[gi])) rt_count(st, rt_mul(v.al, v.lm_step ? v.lm_step[v.perm[gi]] : 0.0));
  }
  return st;
}

// pass 2: the same items again, stored: x_out / lam_out <- (src, lsrc) [+] the step (lam_out and lsrc are indexed by l < L). stepping:
// false leaves every item as it is in src. What is not stepped is written only with copy_rest, which also copies the row's padding: the
// in-place form passes false, and a lane then stores only what it loaded itself, so it needs no barrier.
__device__ __forceinline__ void rt_store(const WinMeta &wm, const StepView &v, int lane, const double *src, const double *lsrc, double *x_out,
                                         double *lam_out, bool stepping, bool copy_rest) {
  const int F = wm.n_frames, cmask = wm.const_mask, L = wm.L;
  int bxo = 0, bso = 0;
  const bool blk_on = lane < 13 && rt_block(lane, F, cmask, bxo, bso);
  if (lane < 13) {
    double out[7];
    if (blk_on && stepping) {
      double s6[6];
      for (int c = 0; c < 6; ++c) s6[c] = rt_mul(v.al, v.step ? v.step[bso + c] : 0.0);
      rt_pose_plus(src + bxo, s6, out);
    } else {
      for (int c = 0; c < 7; ++c) out[c] = src[bxo + c];
    }
    if ((blk_on && stepping) || copy_rest)
      for (int c = 0; c < 7; ++c) x_out[bxo + c] = out[c];
  }
  for (int e = lane; e < RT_EUCLID; e += 64) {
    int xo, so;
    const bool on = rt_euclid(e, F, wm.use_leg, cmask, xo, so) && stepping;
    if (on) x_out[xo] = rt_add(src[xo], rt_mul(v.al, v.step ? v.step[so] : 0.0));
    else if (copy_rest) x_out[xo] = src[xo];
  }
  if (copy_rest && lane < XSTRIDE - (XO_TD + 1)) x_out[XO_TD + 1 + lane] = src[XO_TD + 1 + lane];   // (the row's padding)
  for (int l = lane; l < L; l += 64) {
    const int gi = wm.lm_off + l;
    const bool on = !(v.mask && v.mask[gi]) && stepping;
    if (on) lam_out[l] = rt_add(lsrc[l], rt_mul(v.al, v.lm_step ? v.lm_step[v.perm[gi]] : 0.0));
    else if (copy_rest) lam_out[l] = lsrc[l];
  }
}

}  // namespace
