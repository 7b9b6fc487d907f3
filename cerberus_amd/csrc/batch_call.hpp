// The host frame of a call that queries a resident batch (marginalisation, covariance, residuals, gradient, triangulation, PnP, gyroscope-
// bias alignment, next-frame prediction, dead reckoning and its covariance, gauge fix, failure detection, retraction, set_state, Gauss-Newton step): BatchCall call(ctx, bt, &vilo_ctx::last_X_ms); the call's blocks of device memory, call.lay.take<T>(n); call.begin()
// (one allocation out of the batch's arena, given back when `call` dies); uploads that are not to be timed; call.start(); the copies and
// launches on ctx->stream, at call.ptr<T>(offset); call.finish() (launch errors, the stream drained, last_X_ms written);
// call.down(host, dev, bytes) for every output the caller may have asked for.
// The calls that walk a range of samples per window take their first three blocks and their upload through sample_stream.hpp's SampleUpload.
#pragma once
#include <stddef.h>

namespace vilo {
// Byte offsets of the blocks of one allocation. HIP-free (tests/host_check/batch_call_check.cpp); the only place that knows the alignment.
struct CallLayout {
  // offset of a block of `count` T; a block that is not wanted, or empty, takes no bytes (its offset is where the next block starts)
  template <class T> size_t take(size_t count, bool want = true) {
    const size_t o = at;
    if (want) at = (at + sizeof(T) * count + 255) & ~(size_t)255;
    return o;
  }
  size_t bytes() const { return at; }
  size_t at = 0;
};
}  // namespace vilo

#ifdef __HIPCC__
#include <optional>

#include "batch_state.hpp"

// The blocks of "the batch's records integrated again at x, on copies" (BatchCall::reintegrate). stages 1: records and contact-force
// filters; 2: the prepared records and their flags too. Nothing is taken unless samples are in force on a leg batch.
struct ReintegrationBlocks {
  ReintegrationBlocks(vilo::CallLayout &lay, const BatchDev &bd, int n_stages)
      : on(bd.rp_on && bd.rp_samples && bd.leg), stages(n_stages), NF((size_t)bd.W * 10), o_pre(lay.take<vilo_preint>(NF, on)),
        o_ff(lay.take<double>(VILO_FF_N * NF, on && bd.rp_ff)), o_prep(lay.take<PreintPrepared>(NF, on && stages > 1)),
        o_bad(lay.take<int>(NF, on && stages > 1)) {}
  bool on;
  int stages;
  size_t NF, o_pre, o_ff, o_prep, o_bad;
};

// One call on a resident batch. start / finish / down return what VILO_HIP takes. The arena scope opens at begin(), on the context's
// device: a call that returns before it has touched neither the arena nor the stream, and reports 0 ms, as does one that fails.
struct BatchCall {
  BatchCall(vilo_ctx *c, vilo_batch *b, double vilo_ctx::*ms_) : ctx(c), bt(b), ms(ms_) { ctx->*ms = 0.0; }
  int begin() {
    VILO_HIP(hipSetDevice(ctx->device));
    scope.emplace(ctx, bt);
    base = (char *)scope->alloc(lay.bytes());
    return base ? VILO_OK : VILO_ERR_HIP;   // (ArenaScope::alloc has set ctx->err)
  }
  template <class T> T *ptr(size_t offset) const { return (T *)(base + offset); }
  hipError_t start() { return hipEventRecord(ctx->ev0, ctx->stream); }
  hipError_t finish() {
    float t = 0.f;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(ctx->ev1, ctx->stream);
    if (e == hipSuccess) e = hipEventSynchronize(ctx->ev1);
    if (e == hipSuccess) e = hipEventElapsedTime(&t, ctx->ev0, ctx->ev1);
    if (e == hipSuccess) ctx->*ms = t;
    return e;
  }
  // synchronous download; nothing for an output the caller did not ask for, or an empty one
  hipError_t down(void *host, const void *dev, size_t bytes) { return host && bytes ? hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
  // With samples in force the batch's records may sit at a rejected candidate point: they are integrated again at x by the marginalisation's
  // pass (k_repropagate mode 0; records already integrated there are kept: its own test), with stages 2 followed by the preparation. On
  // copies: `b`, the caller's copy of the batch's BatchDev, is pointed at the blocks of `r`, so the batch's own are never written.
  int reintegrate(BatchDev &b, const ReintegrationBlocks &r) {
    if (!r.on) return VILO_OK;
    const void *pre = b.rp_pre;
    const double *ff = b.rp_ff;
    b.rp_pre = ptr<char>(r.o_pre);
    if (ff) b.rp_ff = ptr<double>(r.o_ff);
    if (r.stages > 1) { b.prep = ptr<PreintPrepared>(r.o_prep); b.prep_bad = ptr<int>(r.o_bad); }
    VILO_HIP(hipMemcpyAsync(b.rp_pre, pre, sizeof(vilo_preint) * r.NF, hipMemcpyDeviceToDevice, ctx->stream));
    if (ff) VILO_HIP(hipMemcpyAsync(b.rp_ff, ff, sizeof(double) * VILO_FF_N * r.NF, hipMemcpyDeviceToDevice, ctx->stream));
    for (int stage = 0; stage < r.stages; ++stage)
      if (vilo_repropagate_launch(ctx, b, 0, stage) != VILO_OK) return VILO_ERR_HIP;
    return VILO_OK;
  }
  vilo_ctx *ctx;
  vilo_batch *bt;
  double vilo_ctx::*ms;
  vilo::CallLayout lay;              // the call's blocks, taken before begin()
  std::optional<ArenaScope> scope;   // (marginalisation sizes a second buffer partway through: scope->alloc)
  char *base = nullptr;
};

// The windows' SolverStates over a vilo_marg_linearize that a query runs: copied aside into a block of the call's memory on the stream
// (`saved`: that copy's status), copied back by restore() or, on a return before it, by the destructor (best effort). Declared after the
// BatchCall, so that the copy back is on the stream before the scope's closing synchronisation.
struct SolverStateGuard {
  SolverStateGuard(BatchCall &call, BatchDev &bd, size_t offset)
      : stream(call.ctx->stream), st(bd.st), aside(call.ptr<SolverState>(offset)), bytes(sizeof(SolverState) * (size_t)bd.W),
        saved(hipMemcpyAsync(aside, st, bytes, hipMemcpyDeviceToDevice, stream)), armed(saved == hipSuccess) {}
  ~SolverStateGuard() { if (armed) (void)restore(); }
  SolverStateGuard(const SolverStateGuard &) = delete;
  hipError_t restore() { armed = false; return hipMemcpyAsync(st, aside, bytes, hipMemcpyDeviceToDevice, stream); }
  hipStream_t stream;
  SolverState *st, *aside;
  size_t bytes;
  hipError_t saved;
  bool armed;
};
#endif
