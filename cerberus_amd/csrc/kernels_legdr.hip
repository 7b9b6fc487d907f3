// Leg-odometry dead reckoning of a frame through samples (vilo_batch_leg_dead_reckon, include/vilo_gpu.h): the nominal-state part of
// IMULegIntegrationBase::midPointIntegration (imu_leg_integration_base.cpp:152-158, :181-351) with propagate()'s carry, without the
// 31 x 31 Jacobian and covariance recurrences vilo_preintegrate / k_repropagate run beside it. The step is legdr_host.hpp's legdr_step,
// the function the CPU path calls too.
//
// One launch, one code path for every batch size (no launch plan; no output depends on the batch a window shares, nor on its position):
//   k_leg_dead_reckon  four lanes per window (lane = leg), sixteen windows per wave, 64 per workgroup of 256. The step's longest stretch
//                      is a leg's forward kinematics and Jacobian (six sin / cos) and its two quaternion rotations: a leg is a lane's
//                      work. delta_q / delta_v are computed redundantly in the four lanes from the same values in the same order, so
//                      they are bitwise equal across the quad. The fused mean needs the four legs' weights and weighted velocities:
//                      every lane takes them from its quad by DPP quad_perm broadcasts (18 doubles a step) and sums them in the fixed order
//                      j = 0 .. 3, so the four lanes hold the same sum_delta_eps bit for bit. No atomics, no LDS; the recurrence
//                      (delta_q, delta_v, the leg's delta_eps, sum_delta_eps, the previous sample's acc / gyr / v / c and the leg's nine
//                      filter values) lives in registers. The call repacks the samples so that what a quad loads in a step is
//                      contiguous (LEGDR_ROW: dt acc gyr, then per leg phi dphi c: 280 bytes); row i + 1 is requested at the top of
//                      step i, ahead of the dependent chain. Quads of a wave leave the loop at different steps; DPP reads stay inside
//                      a quad, whose four lanes make the same number of steps.
//
// Floating-point contraction is off for the whole file, the inlined helpers of vilo_math.hpp and legdr_host.hpp included: the numpy
// definition (tests/leg_dr_model.py) and the host program round every operation, and a trajectory's last row and state_out are the same
// function of the same values.
#pragma clang fp contract(off)
#include <hip/hip_runtime.h>
#include <math.h>

#include "batch_call.hpp"
#include "legdr_host.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_leg_dead_reckon_opts) == 8, "vilo_leg_dead_reckon_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_leg_dead_reckon_record) == 8, "vilo_window_leg_dead_reckon_record: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_sample) == 8 * LEGDR_ROW, "a packed row is a vilo_sample in another order");
static_assert(vilo::LEGDR_FF_N == VILO_FF_N, "the contact-force filter of preint_blocks.hpp's O_FF layout");

#define LEGDR_THREADS 256
#define LEGDR_WINDOWS (LEGDR_THREADS / 4)

struct LegDrArgs {
  int from_frame, pad;
  const double *rows;           // [n_samples][LEGDR_ROW] packed samples
  const int *offsets;           // [W + 1] window w reads rows offsets[w] .. offsets[w + 1]
  const int *step_offsets;      // [W + 1] window w's trajectory rows
  double *state;                // [W][LEGDR_STATE]
  double *legs;                 // [W][LEGDR_LEGS]
  double *traj;                 // [sum n_steps][LEGDR_TRAJ], or null
  vilo_window_leg_dead_reckon_record *rec;   // [W]
};

namespace {

template <int K> __device__ __forceinline__ int quad_bcast_i(int v) { return __builtin_amdgcn_update_dpp(0, v, K * 0x55, 0xf, 0xf, false); }
template <int K> __device__ __forceinline__ double quad_bcast(double v) {
  return __hiloint2double(quad_bcast_i<K>(__double2hiint(v)), quad_bcast_i<K>(__double2loint(v)));
}

// legdr_step's policy of a lane: one leg, the quad's values by DPP
struct LegDrQuadLane {
  static constexpr int N = 1;
  int j;
  __device__ __forceinline__ int leg(int) const { return j; }
  __device__ __forceinline__ bool first() const { return j == 0; }
  __device__ __forceinline__ void gather(const double (&mine)[1], double (&all)[4]) const {
    all[0] = quad_bcast<0>(mine[0]); all[1] = quad_bcast<1>(mine[0]); all[2] = quad_bcast<2>(mine[0]); all[3] = quad_bcast<3>(mine[0]);
  }
  __device__ __forceinline__ bool all_of(bool v) const {
    const int a = v ? 1 : 0;
    return (quad_bcast_i<0>(a) & quad_bcast_i<1>(a) & quad_bcast_i<2>(a) & quad_bcast_i<3>(a)) != 0;
  }
};

}  // namespace

__global__ void __launch_bounds__(LEGDR_THREADS) k_leg_dead_reckon(BatchDev b, const vilo_config *cfgp, LegDrArgs a) {
  using namespace vilo;
  const int win = blockIdx.x * LEGDR_WINDOWS + (threadIdx.x >> 2);
  if (win >= b.W) return;   // (whole quads)
  LegDrQuadLane x;
  x.j = threadIdx.x & 3;
  const vilo_config &cfg = *cfgp;
  const int n_frames = b.win[win].n_frames;
  const int f = a.from_frame < 0 ? n_frames - 1 : a.from_frame;
  const int s_begin = a.offsets[win], n = a.offsets[win + 1] - s_begin;
  const int n_steps = n > 1 ? n - 1 : 0;
  double *state = a.state + (size_t)LEGDR_STATE * win, *legs = a.legs + (size_t)LEGDR_LEGS * win;
  double *traj = a.traj ? a.traj + (size_t)LEGDR_TRAJ * a.step_offsets[win] : nullptr;
  const double *xs = b.x + (size_t)win * XSTRIDE;

  int status = VILO_DR_OK;
  // (f <= VILO_MAX_FRAMES - 1 by the argument check and n_frames <= VILO_MAX_FRAMES: row f of the state exists)
  if (f < 0 || f >= n_frames) status = VILO_DR_NO_FRAME;
  else {
    const double *pose = xs + XO_POSE + 7 * f, *sb = xs + XO_SB + 9 * f, *lb = xs + XO_LB + 4 * f;
    bool finite = legdr_finite(lb[x.j]);
#pragma unroll
    for (int k = 0; k < 7; ++k) finite = finite && legdr_finite(pose[k]);
#pragma unroll
    for (int k = 3; k < 9; ++k) finite = finite && legdr_finite(sb[k]);
    LegDrConst c;
    legdr_const(cfg, sb + 3, sb + 6, c);
    LegDrWorld wf;
    wf.R0 = qR(qnormalized(ldq_pose(pose)));
    wf.P0 = ld3(pose);
    LegDrState<1> s;
    LegDrStep<1> o;
    o.flag[0] = 0.0;
    if (n_steps > 0) {
      const double *row = a.rows + (size_t)LEGDR_ROW * s_begin;
      const double *mine = row + LEGDR_ROW_SHARED + LEGDR_ROW_LEG * x.j;
      // the first sample of the range: (acc_0, gyr_0, phi_0, dphi_0, c_0); its dt is not read
      double sh[LEGDR_ROW_SHARED], lg[1][LEGDR_ROW_LEG];
      sh[0] = 0.0;
#pragma unroll
      for (int k = 1; k < LEGDR_ROW_SHARED; ++k) sh[k] = row[k];
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_LEG; ++k) lg[0][k] = mine[k];
#pragma unroll
      for (int k = 1; k < LEGDR_ROW_SHARED; ++k) finite = finite && legdr_finite(sh[k]);
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_LEG; ++k) finite = finite && legdr_finite(lg[0][k]);
      legdr_start(c, cfg, lb, sh, lg, x, s);
      double nsh[LEGDR_ROW_SHARED], nlg[LEGDR_ROW_LEG];
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_SHARED; ++k) nsh[k] = row[LEGDR_ROW + k];
#pragma unroll
      for (int k = 0; k < LEGDR_ROW_LEG; ++k) nlg[k] = mine[LEGDR_ROW + k];
      for (int i = 1; i < n; ++i) {
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_SHARED; ++k) sh[k] = nsh[k];
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_LEG; ++k) lg[0][k] = nlg[k];
        if (i + 1 < n) {
          // row i + 1, in flight over this step's chain
          const size_t at = (size_t)LEGDR_ROW * (i + 1);
#pragma unroll
          for (int k = 0; k < LEGDR_ROW_SHARED; ++k) nsh[k] = row[at + k];
#pragma unroll
          for (int k = 0; k < LEGDR_ROW_LEG; ++k) nlg[k] = mine[at + k];
        }
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_SHARED; ++k) finite = finite && legdr_finite(sh[k]);
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_LEG; ++k) finite = finite && legdr_finite(lg[0][k]);
        legdr_step(c, s, sh, lg, x, o);
        if (traj) legdr_traj_row(wf, s, o, x, traj + (size_t)LEGDR_TRAJ * (i - 1));
      }
    } else {
      legdr_start(c, cfg, lb, (const double *)nullptr, (const double (*)[LEGDR_ROW_LEG])nullptr, x, s);
    }
    legdr_state_row(wf, s, o.flag, x, state, legs);
    finite = finite && legdr_rows_finite(state, legs, x);
    if (!x.all_of(finite)) status = VILO_DR_NUMERIC;
  }
  if (status != VILO_DR_OK) {
    for (int i = x.j; i < LEGDR_STATE; i += 4) state[i] = 0.0;
    for (int i = x.j; i < LEGDR_LEGS; i += 4) legs[i] = 0.0;
    if (traj)
      for (size_t i = x.j; i < (size_t)LEGDR_TRAJ * n_steps; i += 4) traj[i] = 0.0;
  }
  if (x.first()) {
    vilo_window_leg_dead_reckon_record r;
    r.n_steps = n_steps;
    r.status = status;
    a.rec[win] = r;
  }
}

extern "C" void vilo_default_leg_dead_reckon_opts(vilo_leg_dead_reckon_opts *o) {
  if (!o) return;
  o->from_frame = -1;
  o->reserved = 0;
}

extern "C" int vilo_batch_leg_dead_reckon(vilo_ctx *ctx, vilo_batch *bt, const vilo_leg_dead_reckon_opts *opts, const vilo_sample *samples,
                                          const int32_t *offsets, double *state_out, double *legs_out, double *trajectory_out,
                                          vilo_window_leg_dead_reckon_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_leg_dead_reckon_opts o;
  if (opts) o = *opts; else vilo_default_leg_dead_reckon_opts(&o);
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (const char *what = vilo::leg_dead_reckon_check(o, W, samples, offsets, state_out, legs_out)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_leg_dr_ms);
  if (W == 0) return VILO_OK;
  if (!bt->rec.leg) {
    ctx->err = "vilo_batch_leg_dead_reckon: the batch's windows have no leg factors (use_leg == 0)";
    return VILO_ERR_UNSUPPORTED;
  }
  // packed, before the timed region, into the context's reusable staging: rows | offsets | step offsets
  const size_t n_s = (size_t)offsets[W];
  vilo::CallLayout stage;
  const size_t h_rows = stage.take<double>(LEGDR_ROW * n_s), h_off = stage.take<int32_t>((size_t)W + 1), h_step = stage.take<int32_t>((size_t)W + 1);
  char *host = (char *)vilo_host_stage(ctx, 8, stage.bytes());
  if (!host) {
    ctx->err = "vilo_batch_leg_dead_reckon: no host memory for the packed samples";
    return VILO_ERR_HIP;
  }
  vilo::leg_dead_reckon_pack(samples, n_s, (double *)(host + h_rows));
  memcpy(host + h_off, offsets, sizeof(int32_t) * ((size_t)W + 1));
  const size_t n_rows = (size_t)vilo::dead_reckon_step_offsets(W, offsets, (int32_t *)(host + h_step));
  const bool want_traj = trajectory_out != nullptr;
  // the call's device memory: packed samples | offsets | step offsets | states | legs | trajectory | records
  const size_t o_s = call.lay.take<double>(LEGDR_ROW * n_s), o_o = call.lay.take<int32_t>((size_t)W + 1), o_t = call.lay.take<int32_t>((size_t)W + 1);
  const size_t o_x = call.lay.take<double>(LEGDR_STATE * (size_t)W), o_l = call.lay.take<double>(LEGDR_LEGS * (size_t)W);
  const size_t o_j = call.lay.take<double>(LEGDR_TRAJ * n_rows, want_traj), o_c = call.lay.take<vilo_window_leg_dead_reckon_record>(W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  LegDrArgs a;
  a.from_frame = o.from_frame; a.pad = 0;
  a.rows = call.ptr<double>(o_s);
  a.offsets = call.ptr<int>(o_o);
  a.step_offsets = call.ptr<int>(o_t);
  a.state = call.ptr<double>(o_x);
  a.legs = call.ptr<double>(o_l);
  a.traj = want_traj && n_rows > 0 ? call.ptr<double>(o_j) : nullptr;
  a.rec = call.ptr<vilo_window_leg_dead_reckon_record>(o_c);
  // (not timed; the three host blocks and the three device blocks are laid out alike, so they go up in one copy)
  VILO_HIP(hipMemcpyAsync(call.ptr<char>(o_s), host, h_step + sizeof(int32_t) * ((size_t)W + 1), hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_leg_dead_reckon, dim3((W + LEGDR_WINDOWS - 1) / LEGDR_WINDOWS), dim3(LEGDR_THREADS), 0, ctx->stream, bd,
                     (const vilo_config *)ctx->d_cfg, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(state_out, a.state, sizeof(double) * LEGDR_STATE * (size_t)W));
  VILO_HIP(call.down(legs_out, a.legs, sizeof(double) * LEGDR_LEGS * (size_t)W));
  if (want_traj) VILO_HIP(call.down(trajectory_out, a.traj, sizeof(double) * LEGDR_TRAJ * n_rows));
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_leg_dead_reckon_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_leg_dead_reckon(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, const vilo_window_state *state,
                                           const vilo_leg_dead_reckon_opts *opts, const vilo_sample *samples, const int32_t *offsets,
                                           double *state_out, double *legs_out, double *trajectory_out,
                                           vilo_window_leg_dead_reckon_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_leg_dead_reckon_opts o;
  if (opts) o = *opts; else vilo_default_leg_dead_reckon_opts(&o);
  if (const char *what = vilo::leg_dead_reckon_check(o, n_windows, samples, offsets, state_out, legs_out)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_leg_dead_reckon(ctx, bt, &o, samples, offsets, state_out, legs_out, trajectory_out, records);
  });
}

extern "C" double vilo_last_leg_dead_reckon_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_leg_dr_ms : -1.0; }
