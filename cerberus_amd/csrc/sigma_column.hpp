// Device helpers of the kernels in which lane j of a window's group of lanes holds column j of its covariance (k_dr_covariance: 16 lanes
// a window; k_leg_dr_covariance: 32). The groups of a wave exchange through LDS between themselves only, so what orders them is a
// wavefront fence, and what they agree on they agree by one ballot.
#pragma once
#include <hip/hip_runtime.h>

// stores to LDS by the wave's lanes before it, loads by them after it
__device__ __forceinline__ void sigcol_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Is `finite` true in all LANES lanes of group grp of the wave (the lanes of a group are all here: they entered and left the loop together)
template <int LANES> __device__ __forceinline__ bool sigcol_all_finite(bool finite, int grp) {
  static_assert(LANES == 16 || LANES == 32, "a group is a quarter or a half of a wave");
  const unsigned long long bad = __ballot(!finite);
  return ((bad >> (LANES * grp)) & ((1ull << LANES) - 1)) == 0;
}

// Entry (i, j) and its mirror, i <= j < N, of an N x N row-major matrix from the lane's column j: one triangle feeds both halves
template <int N> __device__ __forceinline__ void sigcol_store_sym(double *dst, const double *c, int j) {
  if (j >= N) return;
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (i <= j) {
      dst[N * i + j] = c[i];
      dst[N * j + i] = c[i];
    }
}

// x_l for an l that differs between lanes. (Values, not the elements themselves: a conditional between two elements of an array is a choice
// of address, and that puts the array in scratch memory.)
__device__ __forceinline__ double sigcol_pick(int l, double x0, double x1, double x2) { return l == 0 ? x0 : (l == 1 ? x1 : x2); }
__device__ __forceinline__ double sigcol_pick(int l, double x0, double x1, double x2, double x3) { return l == 0 ? x0 : (l == 1 ? x1 : (l == 2 ? x2 : x3)); }
