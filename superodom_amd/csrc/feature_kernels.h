// feature_kernels.h -- launchers of feature_kernels.hip: featureExtraction's per-sweep point work on the device
// (laserCloudHandler's ingest, removePointDistortion, uniformFeatureExtraction).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace soicp {

struct DeskewFrames;
struct Pose;

// where the fields of one sensor_msgs::PointCloud2 point are (pcl::fromROSMsg's field match, done by the caller); -1: absent
struct SweepFields {
  uint32_t point_step, row_step, width;
  int32_t x, y, z, intensity, time, ring;
  int32_t ouster;        // 0: velodyne (float time, uint16 ring copied), 1: ouster (T_ouster_sensor, uint32 t in ns, ring 0)
  double ouster_q[4];    // T_ouster_sensor: x y z w
  double ouster_t[3];
};

// where the fields of one livox_ros_driver2 CustomPoint are (all present), livoxHandler's line gate and its rotation
struct LivoxFields {
  uint32_t point_step;
  uint32_t offset_time, x, y, z, reflectivity, tag, line;  // uint32 ns; float; uint8
  uint32_t n_scans;                                        // config_.N_SCANS
  double R[9];                                             // imu_laser_R_Gravity (identity while the IMU buffer is empty), row-major
};

// where the four float fields of a sweep without per-point time are (pcl::fromROSMsg into pcl::PointXYZI; -1: absent), and N_SCANS
struct UntimedFields {
  uint32_t point_step, row_step, width;
  int32_t x, y, z, intensity;
  uint32_t n_scans;  // config_.N_SCANS: 16, 32, 64 take their ring table; 4 and 128 give ring 0 and drop nothing
};

// bytes of one record of either output cloud: point_os::PointcloudXYZITR and pcl::PointXYZI are both 32 bytes
constexpr uint32_t kFeatureRecordBytes = 32;
// surf-sampling candidates per workgroup of the compaction, and the look-back words it needs
constexpr uint32_t kSurfItems = 2048;
inline uint32_t surf_candidates(uint32_t n, uint32_t s) { return n > 1u ? (n - 2u) / s + 1u : 0u; }
inline uint32_t surf_workgroups(uint32_t n, uint32_t s) { return (surf_candidates(n, s) + kSurfItems - 1u) / kSurfItems; }

// payload -> PointcloudXYZITR records (d_rec, 32 B each), de-skewed when n_poses > 0 (d_n_clamped zeroed by the caller)
void launch_ingest_deskew(const uint8_t* d_raw, uint32_t n, const SweepFields& sf, uint8_t* d_rec, double t0, const double* d_poses,
                          uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, hipStream_t s);
// the same for a Livox CustomMsg's points (livoxHandler, :794-806): n points point_step bytes apart, d_raw at any alignment
void launch_livox_ingest_deskew(const uint8_t* d_raw, uint32_t n, const LivoxFields& lf, uint8_t* d_rec, double t0, const double* d_poses,
                                uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, hipStream_t s);
// the same for a sweep without per-point time (assignTimeforPointCloud, :646-708): ring and time computed, the points the
// reference drops or no longer visits left out -- d_rec (room for n) gets the *d_n_kept records that remain, in order.
// d_state (untimed_workgroups words), d_ticket, *d_n_kept and *d_n_clamped zeroed by the caller.
inline uint32_t untimed_workgroups(uint32_t n) { return (n + kSurfItems - 1u) / kSurfItems; }
void launch_untimed_ingest_deskew(const uint8_t* d_raw, uint32_t n, const UntimedFields& uf, uint8_t* d_rec, double t0, const double* d_poses,
                                  uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, uint32_t* d_n_kept, unsigned long long* d_state,
                                  uint32_t* d_ticket, hipStream_t s);
// uniformFeatureExtraction over the records: pcl::PointXYZI records into d_surf, their number into *d_n_surf.
// d_state (surf_workgroups words) and d_ticket zeroed by the caller.
void launch_surf_sample(const uint8_t* d_rec, uint32_t n, uint32_t step, float min_range, uint8_t* d_surf, uint32_t* d_n_surf,
                        unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s);

// laserMapping::publishTopic's registered scan: n records `stride` bytes apart (float x y z at 0 4 8, stride a multiple of 4, d_rec
// 4-byte aligned; not modified) -> the kept ones, transformed, in order and packed at the same stride into d_out (room for n, must not
// overlap d_rec), their number into *d_n_kept.  d_state (registered_scan_workgroups words), d_ticket and *d_n_kept zeroed by the caller.
inline uint32_t registered_scan_workgroups(uint32_t n) { return (n + kSurfItems - 1u) / kSurfItems; }
void launch_registered_scan(const uint8_t* d_rec, uint32_t n, uint32_t stride, const Pose& pose, uint8_t* d_out, uint32_t* d_n_kept,
                            unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s);

}  // namespace soicp
