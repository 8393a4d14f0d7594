// Host build of superodom_amd/csrc/deskew_math.h (the arithmetic of removePointDistortion is host + device code) for the CPU suite:
// tests/deskew_host.py drives it through ctypes.  Built on demand (g++ -O2 -ffp-contract=off).
#include <cstring>

#include "deskew_math.h"

using namespace soicp;

// so_icp_deskew_scan on the host: n records of `stride` bytes (float x y z at 0 4 8, float time at time_off) are rewritten in place
// against n_poses stamped poses; start7 = the sensor frame at the sweep start (t_w_original_l, q_w_original_l).  Returns the number
// of clamped points, or -1 for a table whose times do not increase strictly.  deskew_setup, then deskew_point per record over dev_tab.
extern "C" long long dsk_host_deskew(void* points, size_t n, size_t stride, size_t time_off, double t0, const double* poses, size_t n_poses,
                                     int imu, const double* T_i_l, double* start7) {
  DeskewFrames f;
  std::vector<double> dev_tab;
  double q_sensor[4], t_sensor[3];
  if (!deskew_setup(poses, n_poses, t0, imu, T_i_l, f, dev_tab, q_sensor, t_sensor)) return -1;
  for (int k = 0; k < 3; ++k) start7[k] = t_sensor[k];
  for (int k = 0; k < 4; ++k) start7[3 + k] = q_sensor[k];
  const double* tab = dev_tab.data();
  long long n_clamped = 0;
  for (size_t i = 0; i < n; ++i) {
    char* rec = static_cast<char*>(points) + i * stride;
    float xyz[3], time;
    std::memcpy(xyz, rec, 12);
    std::memcpy(&time, rec + time_off, 4);
    const bool finite = isfinite(xyz[0]) && isfinite(xyz[1]) && isfinite(xyz[2]);
    n_clamped += deskew_point(tab, (uint32_t)n_poses, t0, time, f, xyz[0], xyz[1], xyz[2]) ? 1 : 0;
    if (finite) std::memcpy(rec, xyz, 12);  // (deskew_kernel stores only the points it moved)
  }
  return n_clamped;
}
