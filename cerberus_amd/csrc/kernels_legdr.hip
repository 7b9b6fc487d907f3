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
#include "legdr_quad.hpp"
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

__global__ void __launch_bounds__(LEGDR_THREADS) k_leg_dead_reckon(BatchDev b, const vilo_config *cfgp, LegDrArgs a) {
  using namespace vilo;
  const int win = blockIdx.x * LEGDR_WINDOWS + (threadIdx.x >> 2);
  if (win >= b.W) return;   // (whole quads)
  LegDrQuadLane x;
  x.j = threadIdx.x & 3;
  const vilo_config &cfg = *cfgp;
  const SampleRange rg(b, win, a.from_frame, a.offsets);
  const int n = rg.n;
  double *state = a.state + (size_t)LEGDR_STATE * win, *legs = a.legs + (size_t)LEGDR_LEGS * win;
  double *traj = rg.trajectory(a.traj, LEGDR_TRAJ, a.step_offsets, win);
  const double *xs = b.x + (size_t)win * XSTRIDE;

  bool finite = true;
  if (!rg.no_frame) {
    const double *row = a.rows + (size_t)LEGDR_ROW * rg.s_begin;
    LegDrWalk<1> w;
    finite = legdr_window_start(cfg, xs + XO_POSE + 7 * rg.f, xs + XO_SB + 9 * rg.f, xs + XO_LB + 4 * rg.f, rg.n_steps > 0 ? row : nullptr, x, w);
    if (rg.n_steps > 0) {
      double nsh[LEGDR_ROW_SHARED], nlg[1][LEGDR_ROW_LEG];
      legdr_load_row(row + LEGDR_ROW, 0, x, nsh, nlg);
      for (int i = 1; i < n; ++i) {
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_SHARED; ++k) w.sh[k] = nsh[k];
#pragma unroll
        for (int k = 0; k < LEGDR_ROW_LEG; ++k) w.lg[0][k] = nlg[0][k];
        // row i + 1, in flight over this step's chain
        if (i + 1 < n) legdr_load_row(row + (size_t)LEGDR_ROW * (i + 1), 0, x, nsh, nlg);
        finite = finite && legdr_row_finite(0, x, w.sh, w.lg);
        legdr_step(w.c, w.s, w.sh, w.lg, x, w.o);
        if (traj) legdr_traj_row(w.wf, w.s, w.o, x, traj + (size_t)LEGDR_TRAJ * (i - 1));
      }
    }
    legdr_state_row(w.wf, w.s, w.o.flag, x, state, legs);
    finite = finite && legdr_rows_finite(state, legs, x);
  }
  const int status = rg.status(x.all_of(finite));
  if (status != VILO_DR_OK) {
    legdr_zero_share(x, state, LEGDR_STATE);
    legdr_zero_share(x, legs, LEGDR_LEGS);
    if (traj) legdr_zero_share(x, traj, (size_t)LEGDR_TRAJ * rg.n_steps);
  }
  if (x.first()) rg.record(a.rec, win, status);
}

extern "C" void vilo_default_leg_dead_reckon_opts(vilo_leg_dead_reckon_opts *o) {
  if (!o) return;
  o->from_frame = -1;
  o->reserved = 0;
}

static const char LEG_DR_CALL[] = "vilo_batch_leg_dead_reckon";

extern "C" int vilo_batch_leg_dead_reckon(vilo_ctx *ctx, vilo_batch *bt, const vilo_leg_dead_reckon_opts *opts, const vilo_sample *samples,
                                          const int32_t *offsets, double *state_out, double *legs_out, double *trajectory_out,
                                          vilo_window_leg_dead_reckon_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  const vilo_leg_dead_reckon_opts o = sample_call_opts(opts, vilo_default_leg_dead_reckon_opts);
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  if (const char *what = vilo::leg_dead_reckon_check(o, W, samples, offsets, state_out, legs_out)) return sample_call_fail(ctx, LEG_DR_CALL, what, VILO_ERR_BAD_ARG);
  BatchCall call(ctx, bt, &vilo_ctx::last_leg_dr_ms);
  if (W == 0) return VILO_OK;
  if (!bt->rec.leg) return sample_call_fail(ctx, LEG_DR_CALL, "the batch's windows have no leg factors (use_leg == 0)", VILO_ERR_UNSUPPORTED);
  SampleUpload up(ctx, call, LEG_DR_CALL, W, samples, offsets, LEGDR_ROW, vilo::leg_dead_reckon_pack);
  if (!up.staged()) return VILO_ERR_HIP;
  const size_t n_rows = (size_t)up.n_rows;
  const bool want_traj = trajectory_out != nullptr;
  // the call's device memory after the samples': states | legs | trajectory | records
  const size_t o_x = call.lay.take<double>(LEGDR_STATE * (size_t)W), o_l = call.lay.take<double>(LEGDR_LEGS * (size_t)W);
  const size_t o_j = call.lay.take<double>(LEGDR_TRAJ * n_rows, want_traj), o_c = call.lay.take<vilo_window_leg_dead_reckon_record>(W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  VILO_HIP(up.send(call));
  LegDrArgs a;
  a.from_frame = o.from_frame; a.pad = 0;
  a.rows = up.rows;
  a.offsets = up.offsets;
  a.step_offsets = up.step_offsets;
  a.state = call.ptr<double>(o_x);
  a.legs = call.ptr<double>(o_l);
  a.traj = want_traj && n_rows > 0 ? call.ptr<double>(o_j) : nullptr;
  a.rec = call.ptr<vilo_window_leg_dead_reckon_record>(o_c);
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
  const vilo_leg_dead_reckon_opts o = sample_call_opts(opts, vilo_default_leg_dead_reckon_opts);
  if (const char *what = vilo::leg_dead_reckon_check(o, n_windows, samples, offsets, state_out, legs_out)) return sample_call_fail(ctx, LEG_DR_CALL, what, VILO_ERR_BAD_ARG);
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    return vilo_batch_leg_dead_reckon(ctx, bt, &o, samples, offsets, state_out, legs_out, trajectory_out, records);
  });
}

extern "C" double vilo_last_leg_dead_reckon_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_leg_dr_ms : -1.0; }
