// The host half of vilo_batch_dead_reckon_covariance (include/vilo_gpu.h, kernels_drcov.hip) that needs no device: the argument checks,
// the sizes of the call's blocks and the noise diagonal. The samples are packed and the step offsets formed by deadreckon_host.hpp's
// functions, which this call shares with vilo_batch_dead_reckon. HIP-free (tests/host_check/dr_cov_check.cpp runs it under the address
// and undefined-behaviour sanitizers).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "deadreckon_host.hpp"

namespace vilo {

#define DRC_N 15      // error-state coordinates: dp, dtheta, dv, dba, dbg (IntegrationBase's O_P, O_R, O_V, O_BA, O_BG)
#define DRC_POSE 6    // the pose block of a trajectory row: dp, dtheta
#define DRC_NOISE 6   // 3 x 3 blocks of the 18 x 18 noise diagonal: acc_0, gyr_0, acc_1, gyr_1, acc_w, gyr_w

// What is wrong with the arguments of a call on W windows (null: nothing), without the call's name. Reads offsets[0 .. W], nothing else.
inline const char *dr_cov_check(const vilo_dr_cov_opts &o, int W, const vilo_sample *samples, const int32_t *offsets, const double *state_out,
                                const double *cov_out) {
  return sample_range_check(o.from_frame, o.reserved != 0 ? "reserved must be 0" : nullptr, W, samples, offsets,
                            !state_out ? "state_out is NULL" : (!cov_out ? "cov_out is NULL" : nullptr));
}

// Element counts of the call's arrays on W windows with n_rows steps in all (dead_reckon_step_offsets' sum).
struct DrCovCounts {
  size_t cov, state, traj, rec;   // doubles of cov_in / cov_out, of state_out, of pose_cov_trajectory; records
};
inline DrCovCounts dr_cov_counts(int W, int32_t n_rows) {
  DrCovCounts c;
  const size_t w = W > 0 ? (size_t)W : 0;
  c.cov = (size_t)DRC_N * DRC_N * w;
  c.state = (size_t)DR_STATE * w;
  c.traj = (size_t)DRC_POSE * DRC_POSE * (n_rows > 0 ? (size_t)n_rows : 0);
  c.rec = w;
  return c;
}

// q[DRC_NOISE]: the variance of each 3 x 3 block of the noise diagonal, as vilo_preintegrate_imu builds it (kernels_preint.hip,
// preint_imu_body: "integration_base.h:31-37 (ACC_N on all axes)"): acc_n^2, gyr_n^2, acc_n^2, gyr_n^2, acc_w^2, gyr_w^2. acc_n_z does not
// enter: it belongs to the leg record (vilo_preintegrate).
inline void dr_cov_noise(const vilo_config &cfg, double *q) {
  q[0] = q[2] = cfg.acc_n * cfg.acc_n;
  q[1] = q[3] = cfg.gyr_n * cfg.gyr_n;
  q[4] = cfg.acc_w * cfg.acc_w;
  q[5] = cfg.gyr_w * cfg.gyr_w;
}

}  // namespace vilo
