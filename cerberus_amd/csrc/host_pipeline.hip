// Calls on HOST windows that need nothing of a batch but the public batch calls: one batch through create / solve / download, and the
// pipeline that cuts a large call into sub-batches over several internal contexts (vilo_set_host_pipeline).
#include <algorithm>
#include <thread>

#include "vilo_internal.hpp"

// one batch of host windows through create / solve / download on context c
static int solve_host_batch(vilo_ctx *c, int n, const vilo_window_desc *in, vilo_window_state *inout, const vilo_solve_opts *opts, vilo_solve_summary *out) {
  vilo_batch *bt = nullptr;
  int rc = vilo_batch_create(c, n, in, inout, &bt);
  if (rc != VILO_OK) return rc;
  rc = vilo_batch_solve(c, bt, opts);
  if (rc == VILO_OK) rc = vilo_batch_download(c, bt, inout, out);
  if (rc == VILO_OK && out) {
    for (int w = 0; w < n; ++w)
      if (out[w].termination == 2) rc = VILO_ERR_NUMERIC;
  }
  vilo_batch_destroy(c, bt);
  return rc;
}
static void snapshot_host_states(int n, const vilo_window_desc *in, const vilo_window_state *st, std::vector<double> &keep) {
  size_t tot = 0;
  for (int w = 0; w < n; ++w) tot += (size_t)20 * in[w].n_frames + 15 + (size_t)std::max(0, in[w].n_landmarks);
  keep.resize(tot);
  double *q = keep.data();
  for (int w = 0; w < n; ++w) {
    const int F = in[w].n_frames, L = std::max(0, in[w].n_landmarks);
    const vilo_window_state &s = st[w];
    memcpy(q, s.pose, sizeof(double) * 7 * F); q += 7 * F;
    memcpy(q, s.speed_bias, sizeof(double) * 9 * F); q += 9 * F;
    memcpy(q, s.leg_bias, sizeof(double) * 4 * F); q += 4 * F;
    memcpy(q, s.ex_pose, sizeof(double) * 14); q += 14;
    *q++ = s.td[0];
    if (L > 0) { memcpy(q, s.inv_depth, sizeof(double) * L); q += L; }
  }
}
static void restore_host_states(int n, const vilo_window_desc *in, vilo_window_state *inout, const std::vector<double> &keep) {
  const double *q = keep.data();
  for (int w = 0; w < n; ++w) {
    const int F = in[w].n_frames, L = std::max(0, in[w].n_landmarks);
    vilo_window_state &s = inout[w];
    memcpy(s.pose, q, sizeof(double) * 7 * F); q += 7 * F;
    memcpy(s.speed_bias, q, sizeof(double) * 9 * F); q += 9 * F;
    memcpy(s.leg_bias, q, sizeof(double) * 4 * F); q += 4 * F;
    memcpy(s.ex_pose, q, sizeof(double) * 14); q += 14;
    s.td[0] = *q++;
    if (L > 0) { memcpy(s.inv_depth, q, sizeof(double) * L); q += L; }
  }
}

// A call on many HOST windows (vilo_solve_windows, vilo_optimize_windows), cut into sub-batches that go through `lanes` internal contexts
// of the same device, one host thread each (vilo_set_host_pipeline; default 4 lanes of 1024 windows, from two sub-batches' worth of windows
// up): while one lane's windows are on the DMA engines or in the solver, the other lanes pack theirs — the three resources a hand-over of
// host windows needs (host cores, PCIe, GPU) work at the same time instead of one after the other. The windows are independent and every
// lane solves with the form the whole call would take as ONE batch, so the answer is the one batch's bit for bit
// (tests/test_gpu_parity.py::test_host_pipeline_...). `inout` comes back changed only if every sub-batch came through (or failed
// numerically, which is a per-window outcome): the states a finished sub-batch overwrote are put back.
// Returns false when the call is not one to cut (few windows, pipeline off, per-kernel profiling on): the caller runs it as one batch.
bool vilo_run_on_lanes(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *inout,
                       const std::function<int(vilo_ctx *lane, int w0, int n)> &fn, int *rc_out) {
  const int sub = ctx->pipe_sub, lanes_want = ctx->pipe_lanes;
  if (lanes_want < 2 || sub <= 0 || n_windows < 2 * sub || ctx->profile) return false;
  for (int w = 0; w < n_windows; ++w) {   // (what the snapshots below index with; the sub-batches' own checks say why)
    const vilo_window_state &s = inout[w];
    if (in[w].n_frames < 2 || in[w].n_frames > VILO_MAX_FRAMES || in[w].n_landmarks < 0 || in[w].n_landmarks > VILO_NUM_OF_F || !s.pose || !s.speed_bias || !s.leg_bias ||
        !s.ex_pose || !s.td || (in[w].n_landmarks && !s.inv_depth)) return false;
  }
  // The kernel set of a batch depends on its size and those forms agree to rounding, not bitwise. The lanes run the kernel set of a FULL
  // batch whatever their share (BatchDev::full_regime) with the row form and the solver of the whole call, so a call is cut only if as
  // ONE batch it would certainly be a full one too.
  int with_lm = 0, all_td_const = 1;
  for (int w = 0; w < n_windows; ++w) { with_lm += in[w].n_landmarks > 0 ? 1 : 0; if (!in[w].td_const) all_td_const = 0; }
  if (!vilo::call_is_full_as_one_batch(n_windows, with_lm, vilo::tuning())) return false;
  const bool compact = ctx->compact_rows && all_td_const;
  const int form = vilo::plan_solve({n_windows, with_lm, compact, false, true}, ctx->solver_form, vilo::tuning()).solver;   // what ONE batch of all the windows would be solved with
  const int n_sub = (n_windows + sub - 1) / sub, per = (n_windows + n_sub - 1) / n_sub;   // equal shares: no small tail batch
  const int n_lanes = std::min(lanes_want, n_sub);
  while ((int)ctx->lanes.size() < n_lanes) {
    vilo_ctx *l = nullptr;
    const int rc = vilo_create(&l, &ctx->cfg, ctx->device);
    if (rc != VILO_OK) { ctx->err = "no context for a pipeline lane"; *rc_out = rc; return true; }
    // the lanes pack side by side: each brings its own share of the host's threads (at most the shared pool's 16, at least 2)
    const int hw = (int)std::thread::hardware_concurrency();
    l->dma_turn = &ctx->dma_m;
    l->pool = new vilo::WorkerPool(std::max(2, std::min(16, (hw > 0 ? hw : 1) / std::max(1, lanes_want))) - 1);
    ctx->lanes.push_back(l);
  }
  std::vector<int> rcs(n_sub, VILO_OK);
  std::vector<char> ran(n_sub, 0);
  std::vector<std::vector<double>> keep(n_sub);
  std::vector<double> solve_ms(n_lanes, 0.0), marg_ms(n_lanes, 0.0);
  std::vector<int> general(n_lanes, 0);
  std::vector<std::thread> th;
  for (int li = 0; li < n_lanes; ++li) {
    vilo_ctx *l = ctx->lanes[li];
    l->sqrt_info_mode = ctx->sqrt_info_mode; l->solver_form = form; l->compact_rows = compact ? 1 : 0; l->regime_full = 1;
    l->initial_mu = ctx->initial_mu; l->prior_form = ctx->prior_form; l->err.clear();
  }
  auto lane_work = [&](int li) {
    vilo_ctx *l = ctx->lanes[li];
    for (int i = li; i < n_sub; i += n_lanes) {
      const int w0 = i * per, n = std::min(per, n_windows - w0);
      if (n <= 0) break;
      try {
        snapshot_host_states(n, in + w0, inout + w0, keep[i]);
        l->last_solve_ms = 0.0; l->last_marg_ms = 0.0; l->marg_general_count = 0;
        ran[i] = 1;
        rcs[i] = fn(l, w0, n);
      } catch (...) {   // (host allocation failure inside a lane's thread: reported, not thrown across the C boundary)
        rcs[i] = VILO_ERR_HIP; l->err = "host allocation failed in a pipeline lane";
      }
      solve_ms[li] += l->last_solve_ms; marg_ms[li] += l->last_marg_ms; general[li] += l->marg_general_count;
      if (rcs[i] != VILO_OK && rcs[i] != VILO_ERR_NUMERIC) break;
    }
  };
  std::vector<int> inline_lanes;   // (a lane whose thread the process could not start is worked on this one)
  for (int li = 0; li < n_lanes; ++li) {
    try { th.emplace_back(lane_work, li); } catch (...) { inline_lanes.push_back(li); }
  }
  for (int li : inline_lanes) lane_work(li);
  for (std::thread &t : th) t.join();
  int rc = VILO_OK;
  for (int i = 0; i < n_sub; ++i)
    if (rcs[i] != VILO_OK && rcs[i] != VILO_ERR_NUMERIC) { rc = rcs[i]; ctx->err = ctx->lanes[i % n_lanes]->err; break; }
  if (rc != VILO_OK) {   // a sub-batch was refused or lost its device: the call as a whole did not happen
    for (int i = 0; i < n_sub; ++i) {
      const int w0 = i * per, n = std::min(per, n_windows - w0);
      if (n > 0 && ran[i]) restore_host_states(n, in + w0, inout + w0, keep[i]);
    }
    *rc_out = rc;
    return true;
  }
  ctx->last_solve_ms = 0.0; ctx->last_marg_ms = 0.0; ctx->marg_general_count = 0;
  for (int li = 0; li < n_lanes; ++li) { ctx->last_solve_ms += solve_ms[li]; ctx->last_marg_ms += marg_ms[li]; ctx->marg_general_count += general[li]; }
  for (int i = 0; i < n_sub; ++i) if (rcs[i] == VILO_ERR_NUMERIC) rc = VILO_ERR_NUMERIC;
  *rc_out = rc;
  return true;
}

// Estimator::optimization()'s solve half on host windows (estimator.cpp:1054-1245)
extern "C" int vilo_solve_windows(vilo_ctx *ctx, int n_windows, const vilo_window_desc *in, vilo_window_state *inout,
                                  const vilo_solve_opts *opts, vilo_solve_summary *out) {
  if (!ctx || !in || !inout || !opts || n_windows <= 0) return VILO_ERR_BAD_ARG;
  int rc = VILO_OK;
  if (vilo_run_on_lanes(ctx, n_windows, in, inout, [&](vilo_ctx *l, int w0, int n) { return solve_host_batch(l, n, in + w0, inout + w0, opts, out ? out + w0 : nullptr); }, &rc))
    return rc;
  return solve_host_batch(ctx, n_windows, in, inout, opts, out);
}

// lanes < 2 or sub_windows <= 0: every vilo_solve_windows call is one batch
extern "C" int vilo_set_host_pipeline(vilo_ctx *ctx, int lanes, int sub_windows) {
  if (!ctx || lanes < 0 || lanes > 8 || sub_windows < 0) return VILO_ERR_BAD_ARG;
  ctx->pipe_lanes = lanes; ctx->pipe_sub = sub_windows;
  return VILO_OK;
}
