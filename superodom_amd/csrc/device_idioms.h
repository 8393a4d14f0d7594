// device_idioms.h -- device-side idioms that more than one .hip file needs (private to csrc/; device code only).
#pragma once
#include <hip/hip_runtime.h>

#include "deskew_math.h"

namespace soicp {

// LDS written by some lanes of the wavefront is read by others (and the other way round): orders the accesses in the compiler
// and in the hardware; no instruction of its own beyond the wait it implies
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// Window index of coordinate c along one axis, as LocalMap computes it (LocalMap.h:488-497, :596-605): int((c + 25.0) / 50.0) + origin,
// minus one if c + 25.0 < 0 (truncate, then decrement: c + 25 == -50 k belongs to the cube below).  Without the fp64 division: c + 25.0
// is exact in double and, unless it is an exact multiple of 50, differs from one by at least a float ulp (>= 2^-24 relative), far
// more than the 2^-53 error of multiplying by 0.02; on exact multiples the product rounds to the same integer side.  So the
// truncation is the reference's for every float c whose quotient fits an int.
// One that does not -- NaN, +-inf, |c| beyond 1e11 -- is pinned to x86-64, where the reference runs: the conversion gives INT_MIN there
// and the point, or the query, falls outside the window.  (gfx950's conversion gives 0 for NaN, the origin cube: a NaN point would be
// inserted and leave a NaN centroid in the map, a NaN query would be searched.)
constexpr int kCubeOutsideWindow = -(1 << 30);
__device__ __forceinline__ int cube_coord_f(float c, int origin) {
  const double s = (double)c + 25.0;
  if (!(fabs(s) < 1.0e11)) return kCubeOutsideWindow;
  int i = (int)(s * 0.02) + origin;
  if (s < 0) i--;
  return i;
}

// Adds the number of lanes of the wavefront whose `flag` is set to *counter with one atomic, from the first such lane.  Every lane
// of the wavefront calls it (the ballot is over the active lanes).
__device__ __forceinline__ void wave_count_add(bool flag, uint32_t* counter) {
  const unsigned long long m = __ballot(flag);
  if (m && (threadIdx.x & 63) == (uint32_t)__builtin_ctzll(m)) atomicAdd(counter, (uint32_t)__popcll(m));
}

// The workgroup copies the stamped-pose table (n_poses <= kDeskewLdsPoses entries of kStampedPoseDoubles doubles, deskew_math.h)
// into LDS; the barrier behind it is the caller's.
__device__ __forceinline__ void copy_pose_table(double* tab_lds, const double* __restrict__ poses, uint32_t n_poses) {
  for (uint32_t k = threadIdx.x; k < n_poses * kStampedPoseDoubles; k += blockDim.x) tab_lds[k] = poses[k];
}

}  // namespace soicp
