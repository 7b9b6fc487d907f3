// legdr_host.hpp's policy of a lane that owns one leg of a window whose four legs are the four lanes of a quad (k_leg_dead_reckon,
// k_leg_dr_covariance): the quad's values meet by DPP quad_perm broadcasts, which stay inside a quad. Device only.
#pragma once
#include <hip/hip_runtime.h>

template <int K> __device__ __forceinline__ int quad_bcast_i(int v) { return __builtin_amdgcn_update_dpp(0, v, K * 0x55, 0xf, 0xf, false); }
template <int K> __device__ __forceinline__ double quad_bcast(double v) {
  return __hiloint2double(quad_bcast_i<K>(__double2hiint(v)), quad_bcast_i<K>(__double2loint(v)));
}

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
