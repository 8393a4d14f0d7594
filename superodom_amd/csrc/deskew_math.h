// deskew_math.h -- arithmetic of featureExtraction::removePointDistortion
// (/root/reference/super_odometry/src/FeatureExtraction/featureExtraction.cpp:223-314), shared by the host entry point and
// the HIP kernel.  Transformd products follow include/super_odometry/utils/Twist.h:165-187 through Eigen 3.4's
// quaternion <-> matrix conversions [UPSTREAM Eigen, written out]; slerp is Eigen::QuaternionBase::slerp.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "so_math.h"

namespace soicp {

struct Rigid {     // Transformd: rot (x y z w), pos
  double q[4];
  double t[3];
};

SO_HD void quat_normalized(const double q[4], double o[4]) {  // Eigen 3.4 normalized(): unchanged when the norm is 0
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (n2 > 0) { const double n = sqrt(n2); o[0] = q[0] / n; o[1] = q[1] / n; o[2] = q[2] / n; o[3] = q[3] / n; }
  else { o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3]; }
}
SO_HD void matrix_to_quat(const double a[9], double q[4]) {  // quaternionbase_assign_impl<Matrix3>::run; branches written without indexed registers
  double t = a[0] + a[4] + a[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (a[7] - a[5]) * t; q[1] = (a[2] - a[6]) * t; q[2] = (a[3] - a[1]) * t;
  } else if (!(a[4] > a[0]) && !(a[8] > a[0])) {  // i = 0, j = 1, k = 2
    t = sqrt(a[0] - a[4] - a[8] + 1.0);
    q[0] = 0.5 * t; t = 0.5 / t;
    q[3] = (a[7] - a[5]) * t; q[1] = (a[3] + a[1]) * t; q[2] = (a[6] + a[2]) * t;
  } else if (a[4] > a[0] && !(a[8] > a[4])) {     // i = 1, j = 2, k = 0
    t = sqrt(a[4] - a[8] - a[0] + 1.0);
    q[1] = 0.5 * t; t = 0.5 / t;
    q[3] = (a[2] - a[6]) * t; q[2] = (a[7] + a[5]) * t; q[0] = (a[1] + a[3]) * t;
  } else {                                         // i = 2, j = 0, k = 1
    t = sqrt(a[8] - a[0] - a[4] + 1.0);
    q[2] = 0.5 * t; t = 0.5 / t;
    q[3] = (a[3] - a[1]) * t; q[0] = (a[2] + a[6]) * t; q[1] = (a[5] + a[7]) * t;
  }
}
// Twist::operator* (Twist.h:180-185)
SO_HD Rigid rigid_mul(const Rigid& a, const Rigid& b) {
  double qa[4], qb[4], ra[9], rb[9], rc[9];
  quat_normalized(a.q, qa); quat_normalized(b.q, qb);
  quat_to_matrix(qa, ra); quat_to_matrix(qb, rb);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) rc[3 * i + j] = ra[3 * i] * rb[j] + ra[3 * i + 1] * rb[3 + j] + ra[3 * i + 2] * rb[6 + j];
  Rigid o;
  double q[4];
  matrix_to_quat(rc, q);
  quat_normalized(q, o.q);
  for (int i = 0; i < 3; ++i) o.t[i] = ra[3 * i] * b.t[0] + ra[3 * i + 1] * b.t[1] + ra[3 * i + 2] * b.t[2] + a.t[i];
  return o;
}
// Twist::inverse (Twist.h:165-172)
SO_HD Rigid rigid_inverse(const Rigid& a) {
  Rigid o;
  o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
  double r[9];
  quat_to_matrix(o.q, r);
  for (int i = 0; i < 3; ++i) o.t[i] = -(r[3 * i] * a.t[0] + r[3 * i + 1] * a.t[1] + r[3 * i + 2] * a.t[2]);
  return o;
}
// Eigen::QuaternionBase::slerp
SO_HD void quat_slerp(const double a[4], const double b[4], double t, double o[4]) {
  const double one = 1.0 - 2.220446049250313e-16;
  const double d = a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3];
  const double ad = fabs(d);
  double s0, s1;
  if (ad >= one) { s0 = 1.0 - t; s1 = t; }
  else {
    const double theta = acos(ad), st = sin(theta);
    s0 = sin((1.0 - t) * theta) / st;
    s1 = sin(t * theta) / st;
  }
  if (d < 0) s1 = -s1;
  for (int k = 0; k < 4; ++k) o[k] = s0 * a[k] + s1 * b[k];
}

// one stamped pose of the buffer the scan is de-skewed against: 8 doubles {time, px, py, pz, qx, qy, qz, qw}
constexpr int kStampedPoseDoubles = 8;
// a buffer of up to this many poses is copied into LDS by the kernels that de-skew (device_idioms.h copy_pose_table); a longer
// one is read from global memory
constexpr uint32_t kDeskewLdsPoses = 512;

// getInterpolatedPoseAtTime (featureExtraction.cpp:257-276): the first entry with time > ts is "after"; before the first
// entry its pose is returned; otherwise slerp / lerp between the neighbours.  ts at or beyond the last entry has no
// "after" (the reference dereferences end() there -- it only runs de-skew once a later measurement has arrived,
// :185-201); this restatement returns the last pose and reports the point (*clamped).
template <typename Table>
SO_HD Rigid interpolated_pose(const Table& tab, uint32_t n, double ts, bool* clamped) {
  uint32_t lo = 0, hi = n;  // upper_bound
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (tab[mid * kStampedPoseDoubles] > ts) hi = mid; else lo = mid + 1;
  }
  Rigid r;
  uint32_t at = lo;
  if (at == n) { at = n - 1; *clamped = true; }
  if (at == 0 || lo == n) {
    for (int k = 0; k < 3; ++k) r.t[k] = tab[at * kStampedPoseDoubles + 1 + k];
    for (int k = 0; k < 4; ++k) r.q[k] = tab[at * kStampedPoseDoubles + 4 + k];
    return r;
  }
  const uint32_t b = at - 1;
  const double tb = tab[b * kStampedPoseDoubles], ta = tab[at * kStampedPoseDoubles];
  const double ratio = (ts - tb) / (ta - tb);
  double qb[4], qa[4];
  for (int k = 0; k < 4; ++k) { qb[k] = tab[b * kStampedPoseDoubles + 4 + k]; qa[k] = tab[at * kStampedPoseDoubles + 4 + k]; }
  quat_slerp(qb, qa, ratio, r.q);
  for (int k = 0; k < 3; ++k) r.t[k] = (1 - ratio) * tab[b * kStampedPoseDoubles + 1 + k] + ratio * tab[at * kStampedPoseDoubles + 1 + k];
  return r;
}

struct DeskewFrames {  // per-scan constants (featureExtraction.cpp:279-290)
  Rigid w_original_inv;  // T_w_original.inverse()
  Rigid i_l, l_i;        // T_i_l, T_l_i (src/parameter/parameter.cpp:192-193); used when the pose buffer is the IMU's
  int imu;
};

// the transform applied to a point measured at ts (featureExtraction.cpp:297-306)
template <typename Table>
SO_HD Rigid deskew_transform(const Table& tab, uint32_t n, double ts, const DeskewFrames& f, bool* clamped) {
  const Rigid w_current = interpolated_pose(tab, n, ts, clamped);
  const Rigid original_current = rigid_mul(f.w_original_inv, w_current);
  if (!f.imu) return original_current;
  return rigid_mul(rigid_mul(f.l_i, original_current), f.i_l);
}

// one point of removePointDistortion (:293-306): a finite point measured at t0 + time is moved by deskew_transform (fp64, rounded
// to float); a non-finite one stays.  Used by deskew_kernel and ingest_deskew_kernel alike.  Returns whether the point was clamped.
template <typename Table>
SO_HD bool deskew_point(const Table& tab, uint32_t n, double t0, float time, const DeskewFrames& f, float& x, float& y, float& z) {
  bool clamped = false;
  if (isfinite(x) && isfinite(y) && isfinite(z)) {
    const double ts = (double)time + t0;
    const Rigid T = deskew_transform(tab, n, ts, f, &clamped);
    double ox, oy, oz;
    quat_rotate<double>(T.q, (double)x, (double)y, (double)z, ox, oy, oz);  // Twist::operator*(Tangent3): rot * p + pos
    x = (float)(ox + T.t[0]); y = (float)(oy + T.t[1]); z = (float)(oz + T.t[2]);
  }
  return clamped;
}

// Host side of one de-skew (featureExtraction.cpp:279-290), shared by so_icp_deskew_scan(_dev) and so_icp_extract_features(_dev):
// the per-scan constants, the sensor frame at the sweep start and the pose table the kernels read (positions zeroed for the
// IMU's buffer, extractPose :231-235).  false: the times do not increase strictly (the reference keeps them in a std::map).
inline bool deskew_setup(const double* tab, size_t n_poses, double t0, int imu, const double T_i_l[7], DeskewFrames& f,
                         std::vector<double>& dev_tab, double q_sensor[4], double t_sensor[3]) {
  for (size_t k = 0; k + 1 < n_poses; ++k)
    if (!(tab[k * kStampedPoseDoubles] < tab[(k + 1) * kStampedPoseDoubles])) return false;
  f.imu = imu ? 1 : 0;
  if (T_i_l) { for (int k = 0; k < 3; ++k) f.i_l.t[k] = T_i_l[k]; for (int k = 0; k < 4; ++k) f.i_l.q[k] = T_i_l[3 + k]; }
  else { f.i_l.t[0] = f.i_l.t[1] = f.i_l.t[2] = 0; f.i_l.q[0] = f.i_l.q[1] = f.i_l.q[2] = 0; f.i_l.q[3] = 1; }
  f.l_i = rigid_inverse(f.i_l);  // parameter.cpp:193
  bool clamped_start = false;
  Rigid start = interpolated_pose(tab, (uint32_t)n_poses, t0, &clamped_start);  // :279
  if (imu) start.t[0] = start.t[1] = start.t[2] = 0;                             // extractPose, :231-235
  f.w_original_inv = rigid_inverse(start);
  const Rigid sensor = imu ? rigid_mul(start, f.i_l) : start;                    // :284-290
  for (int k = 0; k < 4; ++k) q_sensor[k] = sensor.q[k];
  for (int k = 0; k < 3; ++k) t_sensor[k] = sensor.t[k];
  dev_tab.assign(tab, tab + n_poses * kStampedPoseDoubles);
  if (imu) for (size_t k = 0; k < n_poses; ++k) dev_tab[k * 8 + 1] = dev_tab[k * 8 + 2] = dev_tab[k * 8 + 3] = 0.0;
  return true;
}

}  // namespace soicp
