// device_idioms.h -- device-side idioms that more than one .hip file needs (private to csrc/; device code only).
#pragma once
#include <hip/hip_runtime.h>

namespace soicp {

// LDS written by some lanes of the wavefront is read by others (and the other way round): orders the accesses in the compiler
// and in the hardware; no instruction of its own beyond the wait it implies
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

}  // namespace soicp
