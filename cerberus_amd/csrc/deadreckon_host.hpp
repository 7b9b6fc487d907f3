// The host half of vilo_batch_dead_reckon (include/vilo_gpu.h, kernels_deadreckon.hip) that needs no device: the argument checks and the
// packing of the samples to the seven doubles the recurrence reads. The range tests and the step offsets are sample_stream.hpp's.
// HIP-free (tests/host_check/dead_reckon_check.cpp runs it under the address and undefined-behaviour sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sample_stream.hpp"

namespace vilo {

#define DR_ROW 7      // doubles of a packed sample: dt, acc (3), gyr (3): 56 bytes of vilo_sample's 280
#define DR_STATE 10   // doubles of a state row: P (3), quaternion x y z w, V (3)

// What is wrong with the arguments of a call on W windows (null: nothing), without the call's name. Reads offsets[0 .. W], nothing else.
inline const char *dead_reckon_check(const vilo_dead_reckon_opts &o, int W, const vilo_sample *samples, const int32_t *offsets, const double *state_out) {
  const char *option = o.write != 0 && o.write != 1 ? "write must be 0 or 1"
                       : o.write && o.from_frame == -1 ? "write needs an explicit from_frame (the frame after a window's last does not exist)"
                                                       : nullptr;
  return sample_range_check(o.from_frame, option, W, samples, offsets, state_out ? nullptr : "state_out is NULL");
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
