// Estimator::optimization() (estimator.cpp:1054-1458) as one call: a batch of the windows, ceres::Solve (vilo_batch_solve), double2vector's
// gauge fix (kernels_gauge.hip), the download, then the marginalisation linearised at that result (kernels_marg.hip). Host code only.
#include <chrono>

#include "batch_state.hpp"

// Estimator::optimization() (estimator.cpp:1054-1458) as one call on one device-resident batch: ceres::Solve, double2vector's
// gauge fix, then the marginalisation linearised at that result.
extern "C" int vilo_optimize_windows_resident(vilo_ctx *ctx, int W, const vilo_window_desc *in, const vilo_resident_refs *refs, vilo_window_state *inout,
                                              const vilo_solve_opts *opts, const int *marginalization_flag, vilo_prior *next_prior,
                                              vilo_solve_summary *summaries) {
  if (!ctx || W <= 0 || !in || !inout || !opts) return VILO_ERR_BAD_ARG;
  if (marginalization_flag && !next_prior) {
    for (int w = 0; w < W; ++w)
      if (!refs || !refs[w].prior_pool) return VILO_ERR_BAD_ARG;
  }
  VILO_HIP(hipSetDevice(ctx->device));
  const bool timing = getenv("VILO_HOST_TIMING") != nullptr;
  auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  const double t0 = now();
  vilo_batch *bt = nullptr;
  int rc = vilo_batch_create_refs(ctx, W, in, refs, inout, &bt);
  if (rc != VILO_OK) return rc;
  const double t1 = now();
  rc = vilo_batch_solve(ctx, bt, opts);
  const double t2 = now();
  if (rc == VILO_OK) rc = vilo_gauge_fix_batch(ctx, bt->d);
  if (rc == VILO_OK) rc = vilo_batch_download(ctx, bt, inout, summaries);
  const double t3 = now();
  if (rc == VILO_OK && marginalization_flag) {
    // the reference only marginalises full windows (estimator.cpp:1243-1244)
    std::vector<int> modes(W);
    for (int w = 0; w < W; ++w) modes[w] = (in[w].n_frames == VILO_MAX_FRAMES) ? marginalization_flag[w] : -1;
    rc = vilo_marginalize_batch(ctx, bt, W, in, refs, inout, modes.data(), next_prior);
  }
  const double t4 = now();
  vilo_batch_destroy(ctx, bt);
  if (timing)
    fprintf(stderr, "[vilo_optimize_windows] W=%d create %.2f ms, solve %.2f ms, gauge fix + download %.2f ms, marginalise %.2f ms (kernels %.2f), destroy %.2f ms\n", W,
            t1 - t0, t2 - t1, t3 - t2, t4 - t3, ctx->last_marg_ms, now() - t4);
  return rc;
}

// The same on host windows without resident references.
extern "C" int vilo_optimize_windows(vilo_ctx *ctx, int W, const vilo_window_desc *in, vilo_window_state *inout, const vilo_solve_opts *opts,
                                     const int *marginalization_flag, vilo_prior *next_prior, vilo_solve_summary *summaries) {
  if (marginalization_flag && !next_prior) return VILO_ERR_BAD_ARG;
  if (!ctx || W <= 0 || !in || !inout || !opts) return VILO_ERR_BAD_ARG;
  // many host windows: sub-batches over the context's pipeline lanes (vilo_set_host_pipeline), like vilo_solve_windows — each window's
  // solve, gauge fix and marginalisation are its own, so the call's results are the one batch's
  int rc = VILO_OK;
  if (vilo_run_on_lanes(ctx, W, in, inout, [&](vilo_ctx *l, int w0, int n) {
        return vilo_optimize_windows_resident(l, n, in + w0, nullptr, inout + w0, opts, marginalization_flag ? marginalization_flag + w0 : nullptr,
                                              next_prior ? next_prior + w0 : nullptr, summaries ? summaries + w0 : nullptr);
      }, &rc))
    return rc;
  return vilo_optimize_windows_resident(ctx, W, in, nullptr, inout, opts, marginalization_flag, next_prior, summaries);
}
