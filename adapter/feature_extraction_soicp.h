// feature_extraction_soicp.h -- feature_extraction_node without rclcpp: the members and the per-sweep sequence of
// super_odometry::featureExtraction (include/super_odometry/FeatureExtraction/featureExtraction.h, src/FeatureExtraction/
// featureExtraction.cpp) for Velodyne and Ouster PointCloud2 sweeps, the per-point work (ingest, de-skew, uniform surf sampling)
// in one so_icp_extract_features call, the LaserFeature published through Outbox as CDR (laser_mapping_soicp.h).
//
// Replaced members: laserCloudHandler (:710-772), manageLidarBuffer (:825-841), synchronize_measurements (:172-219),
// undistortionAndFeatureExtraction (:440-499), extractFeatures (:422-437), publishTopic / publishCloud (:379-420).
// Left to the caller: imu_Handler's integration, imuInit and IMU_INIT (the caller passes stamped orientations and the flag),
// visual_odom_Handler's message parsing (stamped poses), livoxHandler, provide_point_time == 0 (refused here).
// The library has livoxHandler's ingest (so_icp_extract_features_livox, wire/messages.h CustomMsg); this shell does not route a
// sensor: livox configuration to it and keeps refusing it.  The same holds for a sweep without per-point time: the library has
// assignTimeforPointCloud's ingest (so_icp_extract_features_untimed), and this shell keeps refusing provide_point_time: 0 until a
// later change routes it.
#pragma once
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "../include/so_icp.h"
#include "node_config.h"

namespace super_odometry_soicp {

class featureExtraction {
 public:
  // throws std::invalid_argument for a configuration the shell does not restate (provide_point_time 0, a Livox sensor,
  // filter_point_size < 1), before any device state is created; std::runtime_error when the context cannot be created
  featureExtraction(const FeatureConfig& cfg, Outbox* out, int device_id = 0);
  ~featureExtraction();
  featureExtraction(const featureExtraction&) = delete;
  featureExtraction& operator=(const featureExtraction&) = delete;

  // imu_Handler's result (imuBuf.addMeas(imudata, t), :631): the integrated orientation q_w_i (x y z w) at time t
  void addImuOrientation(double t, const double q_xyzw[4]);
  // visual_odom_Handler (visualOdomBuf.addMeas, :642): the odometry pose at its header stamp
  void addVisualOdometry(double t, const double pos[3], const double q_xyzw[4]);
  bool IMU_INIT = false;  // imuInit's flag, owned by the caller

  void laserCloudHandler(const so_wire::PointCloud2& msg);  // the subscription callback

  int frameCount = 0;
  int frames_failed = 0;
  std::string last_error;
  size_t lidar_buffered() const { return lidarBuf.size(); }

 private:
  struct Sweep {
    so_wire::PointCloud2 msg;
    double last_point_time = 0;  // lidar_msg->back().time of the ingested cloud
  };
  template <typename Buf> bool synchronize_measurements(const Buf& measureBuf);
  void manageLidarBuffer(so_wire::PointCloud2&& msg, double timestamp);
  void undistortionAndFeatureExtraction();
  bool extractFeatures(double lidar_start_time, const Sweep& sweep, const std::vector<so_icp_stamped_pose>& poses, bool imu,
                       const double q_w_original[4]);
  void publishTopic(double lidar_start_time, const Sweep& sweep, const so_icp_feature_info& info, const double q_w_original_l[4]);
  double last_time_of(const so_wire::PointCloud2& msg) const;
  bool layout_of(const so_wire::PointCloud2& msg, so_icp_sweep_layout& lay) const;

  FeatureConfig config_;
  Outbox* out_;
  so_icp_ctx* ctx_ = nullptr;
  std::map<double, Sweep> lidarBuf;                  // MapRingBuffer<PointCloud::Ptr>: keyed by the header stamp
  std::map<double, so_icp_stamped_pose> imuBuf;      // MapRingBuffer<Imu::Ptr>: q_w_i, positions 0 (extractPose, :231-235)
  std::map<double, so_icp_stamped_pose> visualOdomBuf;
  double q_w_original_l[4] = {0, 0, 0, 1};           // members set by removePointDistortion (:289-290)
  double t_w_original_l[3] = {0, 0, 0};
  std::vector<uint8_t> nodist_, surf_;               // the message payloads, written by the device
};

}  // namespace super_odometry_soicp
