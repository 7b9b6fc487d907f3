// The frame of a call that walks a window's range of samples from one of its frames: vilo_batch_dead_reckon, _dead_reckon_covariance,
// _leg_dead_reckon and _leg_dead_reckon_covariance (include/vilo_gpu.h). Each takes a flat array of vilo_sample and offsets[W + 1], packs
// the samples to the rows its kernel reads, uploads rows | offsets | step offsets in one copy and runs one kernel in which a window's
// lanes walk rows offsets[w] .. offsets[w + 1] from frame from_frame, leaving a record per window. What the four share is here once; a
// call keeps its options, its outputs, its row format and its kernel.
//   host half    (HIP-free: tests/host_check/ runs it under the sanitizers) the tests of from_frame, offsets and samples; the step
//                offsets; the layout of the three uploaded blocks
//   device half  SampleUpload: the staging, packing and upload of the three blocks; SampleRange: a window's range, status and record as
//                its kernel's lanes see them; the options-and-check preamble of the entry points
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../../include/vilo_gpu.h"
#include "batch_call.hpp"

namespace vilo {

// What is wrong with the arguments of a call on W windows (null: nothing), without the call's name. Reads offsets[0 .. W], nothing else.
// A call hands in what is wrong with its other options (`option`: tested after from_frame, and on no windows too) and with its outputs
// (`output`: tested after offsets, on W > 0 windows).
inline const char *sample_range_check(int from_frame, const char *option, int W, const vilo_sample *samples, const int32_t *offsets, const char *output) {
  if (from_frame < -1 || from_frame > VILO_MAX_FRAMES - 1) return "from_frame must be -1 or 0 .. VILO_MAX_FRAMES - 1";
  if (option) return option;
  if (W <= 0) return nullptr;
  if (!offsets) return "offsets is NULL";
  if (output) return output;
  if (offsets[0] != 0) return "offsets[0] must be 0";
  for (int w = 0; w < W; ++w)
    if (offsets[w + 1] < offsets[w]) return "offsets must not decrease";
  if (offsets[W] > 0 && !samples) return "samples is NULL";
  return nullptr;
}

// step_offsets[0 .. W]: window w's trajectory rows are step_offsets[w] .. step_offsets[w + 1]; a range of n samples is max(0, n - 1)
// steps. Returns their sum (at most offsets[W]: it fits the offsets' type).
inline int32_t dead_reckon_step_offsets(int W, const int32_t *offsets, int32_t *step_offsets) {
  int32_t at = 0;
  step_offsets[0] = 0;
  for (int w = 0; w < W; ++w) {
    const int32_t n = offsets[w + 1] - offsets[w];
    at += n > 1 ? n - 1 : 0;
    step_offsets[w + 1] = at;
  }
  return at;
}

// rows | offsets | step offsets of n_samples samples in rows of row_doubles, taken from `lay`: the host staging and the call's device
// memory both lay the three out through here, which is why one copy of `bytes` from `rows` on carries them all.
struct SampleBlocks {
  size_t rows, offsets, step_offsets, bytes;
};
inline SampleBlocks sample_blocks(CallLayout &lay, int row_doubles, size_t n_samples, int W) {
  SampleBlocks b;
  b.rows = lay.take<double>((size_t)row_doubles * n_samples);
  b.offsets = lay.take<int32_t>((size_t)W + 1);
  b.step_offsets = lay.take<int32_t>((size_t)W + 1);
  b.bytes = b.step_offsets + sizeof(int32_t) * ((size_t)W + 1) - b.rows;
  return b;
}

}  // namespace vilo

#ifdef __HIPCC__
// The options a call runs with: the caller's, or the defaults
template <class Opts> Opts sample_call_opts(const Opts *opts, void (*defaults)(Opts *)) {
  Opts o;
  if (opts) o = *opts; else defaults(&o);
  return o;
}
// vilo_last_error's text of a call that returns `code`
inline int sample_call_fail(vilo_ctx *ctx, const char *name, const char *what, int code) {
  ctx->err = std::string(name) + ": " + what;
  return code;
}

// The samples of a call on W > 0 windows, on their way to the device. Constructed before call.begin(): packs them (pack(samples, n, out),
// not timed) into the context's reusable staging with the offsets and the step offsets, and takes the three device blocks as the call's
// first. staged() fails with ctx->err set. After call.begin(), send() puts the one copy on the stream and points rows, offsets and
// step_offsets at the device blocks.
struct SampleUpload {
  template <class Pack>
  SampleUpload(vilo_ctx *ctx, BatchCall &call, const char *name, int W, const vilo_sample *samples, const int32_t *offsets_in, int row_doubles, Pack pack) {
    const size_t n_s = (size_t)offsets_in[W];
    vilo::CallLayout stage;
    const vilo::SampleBlocks h = vilo::sample_blocks(stage, row_doubles, n_s, W);
    host = (char *)vilo_host_stage(ctx, 8, stage.bytes());
    if (!host) {
      sample_call_fail(ctx, name, "no host memory for the packed samples", VILO_ERR_HIP);
      return;
    }
    pack(samples, n_s, (double *)(host + h.rows));
    memcpy(host + h.offsets, offsets_in, sizeof(int32_t) * ((size_t)W + 1));
    n_rows = vilo::dead_reckon_step_offsets(W, offsets_in, (int32_t *)(host + h.step_offsets));
    host += h.rows;
    dev = vilo::sample_blocks(call.lay, row_doubles, n_s, W);
  }
  bool staged() const { return host != nullptr; }
  hipError_t send(const BatchCall &call) {
    rows = call.ptr<double>(dev.rows);
    offsets = call.ptr<int>(dev.offsets);
    step_offsets = call.ptr<int>(dev.step_offsets);
    return hipMemcpyAsync(call.ptr<char>(dev.rows), host, dev.bytes, hipMemcpyHostToDevice, call.ctx->stream);
  }
  int32_t n_rows = 0;              // steps of all windows: the rows of a trajectory
  const double *rows = nullptr;    // [n_samples][row_doubles]
  const int *offsets = nullptr, *step_offsets = nullptr;   // [W + 1] each
  char *host = nullptr;
  vilo::SampleBlocks dev;
};

// A window's range as the lanes of its kernel see it: the frame it starts from, rows s_begin .. s_begin + n, n_steps = max(0, n - 1).
// (f <= VILO_MAX_FRAMES - 1 by the argument check and n_frames <= VILO_MAX_FRAMES: with !no_frame, row f of the state exists.)
struct SampleRange {
  __device__ __forceinline__ SampleRange(const BatchDev &b, int win, int from_frame, const int *offsets) {
    n_frames = b.win[win].n_frames;
    f = from_frame < 0 ? n_frames - 1 : from_frame;
    s_begin = offsets[win];
    n = offsets[win + 1] - s_begin;
    n_steps = n > 1 ? n - 1 : 0;
    no_frame = f < 0 || f >= n_frames;
  }
  // the window's rows of a trajectory of `row` doubles a step (null: not asked for)
  __device__ __forceinline__ double *trajectory(double *traj, int row, const int *step_offsets, int win) const {
    return traj ? traj + (size_t)row * step_offsets[win] : nullptr;
  }
  __device__ __forceinline__ int status(bool finite) const { return no_frame ? VILO_DR_NO_FRAME : (finite ? VILO_DR_OK : VILO_DR_NUMERIC); }
  // the window's record: one lane's store
  template <class Rec> __device__ __forceinline__ void record(Rec *rec, int win, int status) const {
    Rec r;
    r.n_steps = n_steps;
    r.status = status;
    rec[win] = r;
  }
  int n_frames, f, s_begin, n, n_steps;
  bool no_frame;
};
#endif
