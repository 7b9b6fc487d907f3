// Caller-given local steps on a resident batch's state (vilo_batch_retract, vilo_batch_set_state, vilo_batch_save_state /
// _restore_state, include/vilo_gpu.h): PoseLocalParameterization::Plus (pose_local_parameterization.cpp:12-27) on the pose and extrinsic
// blocks, Ceres' Plus of a Euclidean block on the others, vector2double (estimator.cpp:848-901) for host states, over whole batches.
//
// One launch each, one code path for every batch size; no atomics, no LDS, no output depends on the batch a window shares or on its position:
//   k_retract    one wave per window, x <- x [+] alpha * delta in place (or from the uploaded copy). Lanes 0 .. 12 own the 11 pose and 2
//                extrinsic blocks (vilo::pose_plus, the device function vilo_pose_plus runs); a strided pass covers the 144 Euclidean
//                coordinates (speed-bias 99, leg bias 44, td) and the landmarks (caller order through lm_perm, the mask in device order).
//                Two passes over the same items: the first forms every s = alpha * delta that would be applied, tests it, counts and sums
//                it; a wave-wide vote then decides whether the window is stepped at all; the second forms s again and stores. A lane
//                stores only what it loaded itself, so the in-place form needs no barrier. About 2 KB of state and 8 B per landmark in
//                and out per window: the kernel is paced by memory latency, not by arithmetic.
//   k_set_state  one wave per named window: its packed 240-double row and its inverse depths (device order) copied over the current ones.
//
// The two passes are retract_step.hpp's rt_scan / rt_store, which k_trial_states (kernels_trial.hip) runs too.
// Rounding. s = alpha * delta and x + s are each rounded once (rt_mul / rt_add: contraction off), so numpy restates them to the bit
// (tests/retract_ref.py); pose_plus is compiled as kernels_eval.hip compiles it (the file's default contraction, a function of its own:
// rt_pose_plus), so a pose block is bit for bit vilo_pose_plus(x, s). step_norm's sum of squares is carried in two doubles (TwoSum): the lanes' order of summation leaves no trace
// in it beyond the last bit.
#include <hip/hip_runtime.h>

#include <vector>

#include "batch_call.hpp"
#include "retract_step.hpp"
#include "vilo_math.hpp"

static_assert(sizeof(vilo_retract_opts) == 8, "vilo_retract_opts: 8 bytes (include/vilo_gpu.h)");
static_assert(sizeof(vilo_window_retract_record) == 24, "vilo_window_retract_record: 24 bytes (include/vilo_gpu.h)");

struct RetractArgs {
  const double *state_step;               // [W][RT_STATE], or null
  const double *lm_step;                  // [n_lm] caller order, or null
  const double *alpha;                    // [W], or null
  const unsigned char *mask;              // [n_lm] device order: the landmark mask in force, or null (no mask call yet)
  vilo_window_retract_record *rec;        // [W]
  int uploaded;                           // 1: the step is applied to x0 / lam0
};

__global__ void __launch_bounds__(64) k_retract(BatchDev b, RetractArgs a) {
  const int win = blockIdx.x, lane = threadIdx.x;
  const WinMeta wm = b.win[win];
  const double *src = (a.uploaded ? b.x0 : b.x) + (size_t)win * XSTRIDE, *lsrc = (a.uploaded ? b.lam0 : b.lam) + wm.lm_off;
  StepView v;
  v.step = a.state_step ? a.state_step + (size_t)win * RT_STATE : nullptr;
  v.lm_step = a.lm_step ? a.lm_step + wm.lm_off : nullptr;
  v.mask = a.mask;
  v.perm = b.lm_perm;
  v.al = a.alpha ? a.alpha[win] : 1.0;

  // pass 1: every s that would be applied, tested and summed; nothing is stored
  StepStats st = rt_scan(wm, v, lane);
  const bool numeric = __any(st.bad);   // (wave-wide: the same for every lane, before the window's first store)
  for (int off = 32; off > 0; off >>= 1) {
    const double ph = __shfl_xor(st.hi, off, 64), pl = __shfl_xor(st.lo, off, 64);
    rt_two_sum(st.hi, st.lo, ph, pl);
    st.mx = fmax(st.mx, __shfl_xor(st.mx, off, 64));
    st.n += __shfl_xor(st.n, off, 64);
  }
  if (lane == 0) {
    vilo_window_retract_record r;
    r.status = numeric ? VILO_RETRACT_NUMERIC : VILO_RETRACT_OK;
    r.n_applied = numeric ? 0 : st.n;
    r.step_norm = numeric ? 0.0 : sqrt(rt_add(st.hi, st.lo));
    r.step_max = numeric ? 0.0 : st.mx;
    a.rec[win] = r;
  }
  if (numeric && !a.uploaded) return;   // the window stays as it is

  // pass 2: the same items again, stored. What is not stepped is written only with UPLOADED (the reset's copy).
  rt_store(wm, v, lane, src, lsrc, b.x + (size_t)win * XSTRIDE, b.lam + wm.lm_off, !numeric, a.uploaded != 0);
}

struct SetStateArgs {
  const int *ids;          // [n] the windows named
  const double *rows;      // [n][XSTRIDE] packed as vilo_batch_create packs x0
  const double *lam;       // the named windows' inverse depths, device order, concatenated
  const int *lam_off;      // [n] where window i's start in lam
};

__global__ void __launch_bounds__(64) k_set_state(BatchDev b, SetStateArgs a) {
  const int i = blockIdx.x, lane = threadIdx.x, win = a.ids[i];
  const WinMeta wm = b.win[win];
  for (int k = lane; k < XSTRIDE; k += 64) b.x[(size_t)win * XSTRIDE + k] = a.rows[(size_t)i * XSTRIDE + k];
  for (int l = lane; l < wm.L; l += 64) b.lam[wm.lm_off + l] = a.lam[a.lam_off[i] + l];
}

extern "C" void vilo_default_retract_opts(vilo_retract_opts *o) {
  if (!o) return;
  o->base = VILO_RETRACT_BASE_CURRENT;
  o->reserved = 0;
}

// what is wrong with a retract call's options, or null
static const char *retract_check(const vilo_retract_opts &o) {
  if (o.base != VILO_RETRACT_BASE_CURRENT && o.base != VILO_RETRACT_BASE_UPLOADED) return "vilo_batch_retract: base must be VILO_RETRACT_BASE_CURRENT or VILO_RETRACT_BASE_UPLOADED";
  if (o.reserved != 0) return "vilo_batch_retract: vilo_retract_opts.reserved must be 0 (fill the struct with vilo_default_retract_opts)";
  return nullptr;
}

extern "C" int vilo_batch_retract(vilo_ctx *ctx, vilo_batch *bt, const vilo_retract_opts *opts, const double *state_step, const double *lm_step,
                                  const double *alpha, vilo_window_retract_record *records) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  vilo_retract_opts o;
  if (opts) o = *opts; else vilo_default_retract_opts(&o);
  if (const char *what = retract_check(o)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  if (bt->mask.stale(ctx, "vilo_batch_retract") != VILO_OK) return VILO_ERR_HIP;
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  const size_t n_lm = (size_t)std::max(bd.n_lm, 0);
  BatchCall call(ctx, bt, &vilo_ctx::last_retract_ms);
  if (W == 0) return VILO_OK;
  const bool uploaded = o.base == VILO_RETRACT_BASE_UPLOADED;
  // the call's device memory: state steps | landmark steps | step lengths | records
  const size_t o_s = call.lay.take<double>(RT_STATE * (size_t)W, state_step != nullptr), o_l = call.lay.take<double>(n_lm, lm_step != nullptr && n_lm > 0),
               o_a = call.lay.take<double>(W, alpha != nullptr), o_r = call.lay.take<vilo_window_retract_record>(W);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  RetractArgs a;
  a.state_step = state_step ? call.ptr<double>(o_s) : nullptr;
  a.lm_step = lm_step && n_lm > 0 ? call.ptr<double>(o_l) : nullptr;
  a.alpha = alpha ? call.ptr<double>(o_a) : nullptr;
  a.mask = bt->mask.d_mask;
  a.rec = call.ptr<vilo_window_retract_record>(o_r);
  a.uploaded = uploaded ? 1 : 0;
  // (not timed)
  if (a.state_step) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_s), state_step, sizeof(double) * RT_STATE * (size_t)W, hipMemcpyHostToDevice, ctx->stream));
  if (a.lm_step) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_l), lm_step, sizeof(double) * n_lm, hipMemcpyHostToDevice, ctx->stream));
  if (a.alpha) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_a), alpha, sizeof(double) * (size_t)W, hipMemcpyHostToDevice, ctx->stream));
  // (UPLOADED: what vilo_batch_reset restores besides x and lam)
  if (uploaded && bd.rp_on && bt->rec.rp_ff0 && ctx->cfg.contact_sensor_type == 2)
    VILO_HIP(hipMemcpyAsync(bt->rec.rp_ff, bt->rec.rp_ff0, sizeof(double) * (size_t)W * 10 * VILO_FF_N, hipMemcpyDeviceToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_retract, dim3(W), dim3(64), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());
  VILO_HIP(call.down(records, a.rec, sizeof(vilo_window_retract_record) * (size_t)W));
  return VILO_OK;
}

extern "C" int vilo_window_retract(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *state, const vilo_retract_opts *opts,
                                   const double *state_step, const double *lm_step, const double *alpha, vilo_window_retract_record *records) {
  if (!ctx || n_windows < 1 || !in || !state) return VILO_ERR_BAD_ARG;
  vilo_retract_opts o;
  if (opts) o = *opts; else vilo_default_retract_opts(&o);
  if (const char *what = retract_check(o)) {
    ctx->err = what;
    return VILO_ERR_BAD_ARG;
  }
  return vilo_with_batch(ctx, n_windows, in, state, [&](vilo_batch *bt) {
    const int r = vilo_batch_retract(ctx, bt, &o, state_step, lm_step, alpha, records);
    if (r != VILO_OK) return r;
    return vilo_batch_download(ctx, bt, state, nullptr);
  });
}

extern "C" double vilo_last_retract_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_retract_ms : -1.0; }

extern "C" int vilo_batch_set_state(vilo_ctx *ctx, vilo_batch *bt, int n, const int32_t *window_ids, const vilo_window_state *state) {
  if (!ctx || !bt || n < 1 || !window_ids || !state) return VILO_ERR_BAD_ARG;
  const BatchDev &bd = bt->d;
  const int W = bd.W;
  std::vector<unsigned char> named((size_t)std::max(W, 0), 0);
  for (int i = 0; i < n; ++i) {
    const int w = window_ids[i];
    if (w < 0 || w >= W) { ctx->err = "vilo_batch_set_state: a window id is outside 0 .. W - 1"; return VILO_ERR_BAD_ARG; }
    if (named[w]) { ctx->err = "vilo_batch_set_state: a window id is named twice"; return VILO_ERR_BAD_ARG; }
    named[w] = 1;
    const vilo_window_state &s = state[i];
    if (!s.pose || !s.speed_bias || !s.leg_bias || !s.ex_pose || !s.td || (bt->lm.L[w] > 0 && !s.inv_depth)) {
      ctx->err = "vilo_batch_set_state: a state array is NULL";
      return VILO_ERR_BAD_ARG;
    }
  }
  BatchCall call(ctx, bt, &vilo_ctx::last_set_state_ms);
  VILO_HIP(hipSetDevice(ctx->device));
  std::vector<WinMeta> wins((size_t)W);   // (n_frames of the named windows: the host keeps no copy)
  VILO_HIP(hipMemcpy(wins.data(), bd.win, sizeof(WinMeta) * (size_t)W, hipMemcpyDeviceToHost));
  // the named windows as fill_window (batch_pack.hpp) packs x0 and lam0
  std::vector<double> rows((size_t)n * XSTRIDE, 0.0), lam;
  std::vector<int> ids((size_t)n), lam_off((size_t)n);
  const BatchLandmarks &lm = bt->lm;
  for (int i = 0; i < n; ++i) {
    const int w = window_ids[i], F = wins[w].n_frames;
    const vilo_window_state &s = state[i];
    double *xw = &rows[(size_t)i * XSTRIDE];
    memcpy(xw + XO_POSE, s.pose, sizeof(double) * 7 * F);
    memcpy(xw + XO_SB, s.speed_bias, sizeof(double) * 9 * F);
    memcpy(xw + XO_LB, s.leg_bias, sizeof(double) * 4 * F);
    for (int k = F; k < VILO_MAX_FRAMES; ++k) xw[XO_POSE + 7 * k + 6] = 1.0;
    memcpy(xw + XO_EX, s.ex_pose, sizeof(double) * 14);
    xw[XO_TD] = s.td[0];
    ids[i] = w;
    lam_off[i] = (int)lam.size();
    for (int l = 0; l < lm.L[w]; ++l) lam.push_back(s.inv_depth[lm.perm[lm.lm_off[w] + l]]);
  }
  // the call's device memory: ids | rows | inverse depths | their offsets
  const size_t o_i = call.lay.take<int>(n), o_x = call.lay.take<double>(rows.size()), o_l = call.lay.take<double>(lam.size(), !lam.empty()),
               o_o = call.lay.take<int>(n);
  if (call.begin() != VILO_OK) return VILO_ERR_HIP;
  SetStateArgs a;
  a.ids = call.ptr<int>(o_i); a.rows = call.ptr<double>(o_x); a.lam = call.ptr<double>(o_l); a.lam_off = call.ptr<int>(o_o);
  VILO_HIP(hipMemcpyAsync(call.ptr<int>(o_i), ids.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_x), rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice, ctx->stream));
  if (!lam.empty()) VILO_HIP(hipMemcpyAsync(call.ptr<double>(o_l), lam.data(), sizeof(double) * lam.size(), hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(hipMemcpyAsync(call.ptr<int>(o_o), lam_off.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
  VILO_HIP(call.start());
  hipLaunchKernelGGL(k_set_state, dim3(n), dim3(64), 0, ctx->stream, bd, a);
  VILO_HIP(call.finish());   // (the stream is drained: the host vectors may go)
  return VILO_OK;
}

extern "C" double vilo_last_set_state_ms(const vilo_ctx *ctx) { return ctx ? ctx->last_set_state_ms : -1.0; }

extern "C" int vilo_batch_save_state(vilo_ctx *ctx, vilo_batch *bt) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  return bt->snap.save(ctx, bt->arena, bt->d);
}

extern "C" int vilo_batch_restore_state(vilo_ctx *ctx, vilo_batch *bt) {
  if (!ctx || !bt) return VILO_ERR_BAD_ARG;
  VILO_HIP(hipSetDevice(ctx->device));
  return bt->snap.restore(ctx, bt->d);
}
