// The host half of vilo_batch_dead_reckon (include/vilo_gpu.h, kernels_deadreckon.hip) that needs no device: the argument checks, the
// windows' step offsets and the packing of the samples to the seven doubles the recurrence reads. HIP-free
// (tests/host_check/dead_reckon_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/vilo_gpu.h"

namespace vilo {

#define DR_ROW 7      // doubles of a packed sample: dt, acc (3), gyr (3): 56 bytes of vilo_sample's 280
#define DR_STATE 10   // doubles of a state row: P (3), quaternion x y z w, V (3)

// What is wrong with the arguments of a call on W windows (null: nothing). Reads offsets[0 .. W], nothing else.
inline const char *dead_reckon_check(const vilo_dead_reckon_opts &o, int W, const vilo_sample *samples, const int32_t *offsets, const double *state_out) {
  if (o.from_frame < -1 || o.from_frame > VILO_MAX_FRAMES - 1) return "vilo_batch_dead_reckon: from_frame must be -1 or 0 .. VILO_MAX_FRAMES - 1";
  if (o.write != 0 && o.write != 1) return "vilo_batch_dead_reckon: write must be 0 or 1";
  if (o.write && o.from_frame == -1) return "vilo_batch_dead_reckon: write needs an explicit from_frame (the frame after a window's last does not exist)";
  if (W <= 0) return nullptr;
  if (!offsets) return "vilo_batch_dead_reckon: offsets is NULL";
  if (!state_out) return "vilo_batch_dead_reckon: state_out is NULL";
  if (offsets[0] != 0) return "vilo_batch_dead_reckon: offsets[0] must be 0";
  for (int w = 0; w < W; ++w)
    if (offsets[w + 1] < offsets[w]) return "vilo_batch_dead_reckon: offsets must not decrease";
  if (offsets[W] > 0 && !samples) return "vilo_batch_dead_reckon: samples is NULL";
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

// out[n][DR_ROW] = dt, acc, gyr of samples[0 .. n)
inline void dead_reckon_pack(const vilo_sample *samples, size_t n, double *out) {
  for (size_t i = 0; i < n; ++i) {
    double *r = out + DR_ROW * i;
    const vilo_sample &s = samples[i];
    r[0] = s.dt;
    r[1] = s.acc[0]; r[2] = s.acc[1]; r[3] = s.acc[2];
    r[4] = s.gyr[0]; r[5] = s.gyr[1]; r[6] = s.gyr[2];
  }
}

}  // namespace vilo
