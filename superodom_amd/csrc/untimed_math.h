// untimed_math.h -- arithmetic of featureExtraction::assignTimeforPointCloud (src/FeatureExtraction/featureExtraction.cpp:646-708),
// the ingest of a sweep without per-point time (provide_point_time: 0): the ring from the elevation angle, the drop test and the
// time from the point's index.  Shared by the kernel and host code, expression for expression; every operation is written with
// the type the C++ expression gives it (float overloads of sqrt and atan assumed).
#pragma once
#include "so_math.h"

namespace soicp {

// float angle = atan(z / sqrt(x * x + y * y)) * 180 / M_PI  (:661): the sum, sqrt and the quotient in float; atan as float,
// defined as the correctly rounded value (fp64 atan, rounded once); * 180 a float product; / M_PI in double; rounded to float.
// sqrtf and the plain quotient are correctly rounded on the host and, in a build without fast-math (build.py), on the device:
// there sqrtf is v_sqrt_f32 with the +-1 ulp fma fix-up and the quotient the v_div_scale / v_div_fmas / v_div_fixup sequence
// (DESIGN section 9).  __fsqrt_rn is not used: in this toolchain it is the bare 1 ulp v_sqrt_f32.
SO_HD float untimed_angle(float x, float y, float z) {
  const float a = (float)atan((double)(z / sqrtf(x * x + y * y)));
  return (float)((double)(a * 180.0f) / 3.14159265358979323846);
}

constexpr int kUntimedDropped = -1;

// scanID of :664-699 for config_.N_SCANS == n_scans, or kUntimedDropped where the loop does cloud_size--; continue.
// int(NaN) is pinned to x86-64's INT_MIN, so a NaN angle is dropped in the three tables; any other n_scans (4, 128) is the
// "wrong scan number" branch: ring 0, nothing dropped.
SO_HD int untimed_ring(float angle, int n_scans) {
  if (n_scans != 16 && n_scans != 32 && n_scans != 64) return 0;
  if (angle != angle) return kUntimedDropped;
  int id;
  if (n_scans == 16) {
    id = (int)((double)((angle + 15.0f) / 2.0f) + 0.5);
    if (id > 15 || id < 0) return kUntimedDropped;
  } else if (n_scans == 32) {
    id = (int)(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
    if (id > 31 || id < 0) return kUntimedDropped;
  } else {
    if ((double)angle >= -8.83) id = (int)((double)(2.0f - angle) * 3.0 + 0.5);
    else id = 32 + (int)((-8.83 - (double)angle) * 2.0 + 0.5);
    if (angle > 2.0f || (double)angle < -24.33 || id > 50 || id < 0) return kUntimedDropped;
  }
  return id;
}

// :701-703 with featureExtraction.h:91-93; i is the point's index in the incoming sweep, whatever was dropped in front of it
SO_HD float untimed_time(uint32_t i, uint32_t n_scans) {
  const double scanPeriod = 0.100859904 - 20.736e-6, columnTime = 55.296e-6, laserTime = 2.304e-6;
  const float rel = (float)((columnTime * (double)(int)(i / n_scans) + laserTime * (double)(i % n_scans)) / scanPeriod);
  return (float)((double)rel * scanPeriod);
}

}  // namespace soicp
