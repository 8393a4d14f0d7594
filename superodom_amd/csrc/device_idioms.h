// device_idioms.h -- device-side idioms that more than one .hip file needs (private to csrc/; device code only).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

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

// nanoflann::L2Distance::compute, flann/octree.h:93-102: float differences, squares and sum in double
// (std::pow(float,int) promotes), narrowed to float.  (The k-NN sweeps of kernels.hip and the geometry export of
// corr_geometry_kernels.hip; moved here from kernels.hip as it stands.)
__device__ __forceinline__ float l2_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float dx = qx - px, dy = qy - py, dz = qz - pz;
  return (float)((double)dx * (double)dx + (double)dy * (double)dy + (double)dz * (double)dz);
}

// ---- launch entry: fetch what the first statements of a kernel read in one memory trip per batch (arguments, then state)
// A launch starts cold: its kernel-argument segment was just written by the host side and its state block by the launch in front
// (the scalar cache is invalidated between kernels).  The compiler sinks every argument load to its first use, and the early
// returns of a kernel keep its state loads apart, so the entry code touches those lines one after the other, one trip each.  The
// helpers below load one dword of every 64-byte line of a byte range, together, and drop the values: the code behind them finds its
// lines in the scalar cache.  The addresses are wave-uniform, so the loads are scalar loads; nothing is stored, nothing stays live.

// Bytes of the explicit arguments of a kernel, laid out as the kernel-argument segment lays them out (each at its natural alignment).
template <typename... A>
struct KernargExtent;
template <>
struct KernargExtent<> { static constexpr size_t at(size_t off) { return off; } };
template <typename T, typename... A>
struct KernargExtent<T, A...> {
  static constexpr size_t at(size_t off) { return KernargExtent<A...>::at((off + alignof(T) - 1) / alignof(T) * alignof(T) + sizeof(T)); }
};
template <typename F>
struct KernargBytes;
template <typename... A>
struct KernargBytes<void (*)(A...)> { static constexpr size_t value = KernargExtent<A...>::at(0); };

// OR of one dword per 64-byte line that the BYTES bytes at p overlap, whatever p's alignment beyond 4: the dwords at 0, 64, 128, ...
// and the last one (a line that begins inside the range holds one of the former, or begins after the last of them and holds the latter)
template <size_t BYTES, typename P>
__device__ __forceinline__ uint32_t touch_lines(P p) {
  static_assert(BYTES >= 4 && BYTES % 4 == 0, "whole dwords: never a byte beyond the range");
  uint32_t x = p[BYTES / 4 - 1];
#pragma unroll
  for (size_t o = 0; o + 4 <= BYTES; o += 64) x |= p[o / 4];
  return x;
}
// The values are not needed, the loads are.  after_loaded takes them in a scalar register through an empty statement and hands back
// the pointer the code behind it goes on with, plus a zero the compiler cannot see through: the statement survives because that
// pointer is used, and the loads of that code cannot be issued before the statement's wait.  Not volatile on purpose -- a volatile
// statement counts as a possible store, and behind it the uniform loads through every pointer that is not read-only to the kernel
// become vector loads.  (The pointer itself through the statement would lose its address space: flat loads.)
template <typename T>
__device__ __forceinline__ T* after_loaded(T* p, uint32_t x) {
  uint32_t zero = 0;
  asm("" : "+s"(zero) : "s"(x));
  using Byte = std::conditional_t<std::is_const<T>::value, const char, char>;
  return reinterpret_cast<T*>(reinterpret_cast<Byte*>(p) + zero);
}

// one dword per line of the explicit arguments of the calling kernel: kernarg_lines<decltype(&this_kernel<...>)>()
template <typename F>
__device__ __forceinline__ uint32_t kernarg_lines() {
  constexpr size_t bytes = KernargBytes<F>::value;
  static_assert(bytes % 4 == 0 && bytes <= 4096, "explicit kernel arguments: whole dwords, within the segment");
  typedef const __attribute__((address_space(4))) uint32_t* KernargWords;
  // (+ the grid size, which the segment holds behind the explicit arguments, possibly on a line of its own: read the way every
  //  kernel reads it, not by address -- nothing beyond the explicit arguments is addressed here)
  return touch_lines<bytes>((KernargWords)__builtin_amdgcn_kernarg_segment_ptr()) | gridDim.x;
}
// the fields FIRST .. LAST (both included, in declaration order) of the block at st
#define SO_WARM_FIELDS(st, T, FIRST, LAST)                                                                                    \
  touch_lines<offsetof(T, LAST) + sizeof(T::LAST) - offsetof(T, FIRST)>(                                                       \
      reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(st) + offsetof(T, FIRST)))

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

// surf_sample_kernel's decoupled look-back as a function, for registered_scan_kernel (feature_kernels.hip)
// and correspondences_kernel (corr_kernels.hip): run by the first wavefront of workgroup
// `bid` (ticket order) once it knows `agg`, the number it keeps.  Records = flag << 62 | value (flag 1: this workgroup's own count,
// 2: the count up to and including it), all zero before the launch, vector atomics at agent scope.  Publishes agg, walks back 64
// records at a time until a flag-2 record, publishes the inclusive count and returns the number kept in front of the workgroup
// (on every lane).  surf_sample_kernel keeps its own copy in line: calling this from it changes its register allocation and
// instruction order, and that kernel's code stays as measured.
__device__ __forceinline__ uint32_t lookback_exclusive(unsigned long long* state, uint32_t bid, uint32_t agg, int lane) {
  if (lane == 0) __hip_atomic_store(&state[bid], ((bid == 0u ? 2ull : 1ull) << 62) | (unsigned long long)agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t excl = 0;
  int base = (int)bid - 1;
  while (base >= 0) {
    const int j = base - lane;
    unsigned long long r = 2ull << 62;
    if (j >= 0) {
      do { r = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((r >> 62) == 0ull);
    }
    const unsigned long long mi = __ballot((r >> 62) == 2ull);
    const int first = mi ? __ffsll((long long)mi) - 1 : 64;
    uint32_t contrib = lane <= first ? (uint32_t)(r & 0xFFFFFFFFull) : 0u;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) contrib += (uint32_t)__shfl_xor((int)contrib, d, 64);
    excl += contrib;
    if (mi) break;
    base -= 64;
  }
  if (lane == 0 && bid != 0u) __hip_atomic_store(&state[bid], (2ull << 62) | (unsigned long long)(excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return excl;
}

}  // namespace soicp
