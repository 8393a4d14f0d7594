// feature_extraction_soicp.cpp -- see feature_extraction_soicp.h.  Citations: src/FeatureExtraction/featureExtraction.cpp.
#include "feature_extraction_soicp.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

namespace super_odometry_soicp {

featureExtraction::featureExtraction(const FeatureConfig& cfg, Outbox* out, int device_id) : config_(cfg), out_(out) {
  // assignTimeforPointCloud (:670-708) is not restated: no shipped config sets it, and its ring rejection uses atan in float
  if (config_.provide_point_time == 0)
    throw std::invalid_argument("feature_extraction_node.provide_point_time: 0 is not supported (the sweep must carry per-point times)");
  if (config_.sensor != SensorType::VELODYNE && config_.sensor != SensorType::OUSTER)
    throw std::invalid_argument("sensor: '" + config_.sensor_name + "' is not supported (velodyne or ouster; livox CustomMsg ingest is not restated)");
  if (config_.filter_point_size < 1) throw std::invalid_argument("feature_extraction_node.filter_point_size must be >= 1");
  if (config_.skipFrame < 1) throw std::invalid_argument("feature_extraction_node.mapping_skip_frame must be >= 1");
  so_icp_config c;
  so_icp_default_config(&c);
  c.device_id = device_id;
  ctx_ = so_icp_create(&c);
  if (!ctx_) throw std::runtime_error(std::string("so_icp_create: ") + so_icp_last_error(nullptr));
}

featureExtraction::~featureExtraction() { if (ctx_) so_icp_destroy(ctx_); }

void featureExtraction::addImuOrientation(double t, const double q[4]) {
  so_icp_stamped_pose p{};
  p.time = t;
  for (int k = 0; k < 4; ++k) p.rot[k] = q[k];
  imuBuf.emplace(t, p);  // (std::map::insert: a second measurement at the same stamp is dropped, as MapRingBuffer::addMeas does)
}

void featureExtraction::addVisualOdometry(double t, const double pos[3], const double q[4]) {
  so_icp_stamped_pose p{};
  p.time = t;
  for (int k = 0; k < 3; ++k) p.pos[k] = pos[k];
  for (int k = 0; k < 4; ++k) p.rot[k] = q[k];
  visualOdomBuf.emplace(t, p);
}

// pcl::detail::FieldMatches: name, datatype, count 1 (or 0 for a single value); the first match
static int32_t field_offset(const so_wire::PointCloud2& m, const char* name, uint8_t type) {
  for (const auto& f : m.fields)
    if (f.name == name && f.datatype == type && (f.count == 1 || f.count == 0)) return (int32_t)f.offset;
  return -1;
}

bool featureExtraction::layout_of(const so_wire::PointCloud2& m, so_icp_sweep_layout& lay) const {
  using PF = so_wire::PointField;
  std::memset(&lay, 0, sizeof(lay));
  const bool ouster = config_.sensor == SensorType::OUSTER;
  lay.sensor = ouster ? SO_ICP_SENSOR_OUSTER : SO_ICP_SENSOR_VELODYNE;
  lay.is_bigendian = m.is_bigendian ? 1 : 0;
  lay.point_step = m.point_step; lay.row_step = m.row_step;
  lay.off_x = field_offset(m, "x", PF::FLOAT32); lay.off_y = field_offset(m, "y", PF::FLOAT32); lay.off_z = field_offset(m, "z", PF::FLOAT32);
  lay.off_intensity = field_offset(m, "intensity", PF::FLOAT32);
  lay.off_time = ouster ? field_offset(m, "t", PF::UINT32) : field_offset(m, "time", PF::FLOAT32);
  lay.off_ring = ouster ? -1 : field_offset(m, "ring", PF::UINT16);
  lay.filter_point_size = config_.filter_point_size;
  lay.min_range = config_.min_range;
  for (int k = 0; k < 7; ++k) lay.T_ouster_sensor[k] = config_.T_ouster_sensor[k];
  return (uint64_t)m.row_step * (m.height ? m.height - 1 : 0) + (uint64_t)m.width * m.point_step <= m.data.size() || !m.width || !m.height;
}

// lidar_msg->back().time of the ingested cloud (the time field of the last point; 0 when it has no match)
double featureExtraction::last_time_of(const so_wire::PointCloud2& m) const {
  so_icp_sweep_layout lay;
  if (!m.width || !m.height || !layout_of(m, lay) || lay.off_time < 0 || (uint32_t)lay.off_time + 4 > m.point_step) return 0.0;
  const size_t at = (size_t)(m.height - 1) * m.row_step + (size_t)(m.width - 1) * m.point_step + (size_t)lay.off_time;
  if (lay.sensor == SO_ICP_SENSOR_OUSTER) {
    uint32_t t;
    std::memcpy(&t, m.data.data() + at, 4);
    return (double)((float)t * 1e-9f);  // dst.time = src.t * 1e-9f
  }
  float t;
  std::memcpy(&t, m.data.data() + at, 4);
  return (double)t;
}

// manageLidarBuffer (:825-841): at most 50 sweeps, the oldest dropped first
void featureExtraction::manageLidarBuffer(so_wire::PointCloud2&& msg, double timestamp) {
  while (lidarBuf.size() >= 50) lidarBuf.erase(lidarBuf.begin());
  Sweep s;
  s.last_point_time = last_time_of(msg);
  s.msg = std::move(msg);
  lidarBuf.emplace(timestamp, std::move(s));
}

// synchronize_measurements (:172-219)
template <typename Buf> bool featureExtraction::synchronize_measurements(const Buf& measureBuf) {
  if (lidarBuf.empty() || measureBuf.empty()) return false;
  const double lidar_start_time = lidarBuf.begin()->first;
  const double lidar_end_time = lidar_start_time + lidarBuf.begin()->second.last_point_time;
  const double meas_start_time = measureBuf.begin()->first, meas_end_time = measureBuf.rbegin()->first;
  if (meas_end_time <= lidar_end_time) return false;  // the measurements have not caught up with the sweep
  if (meas_start_time >= lidar_start_time) {         // the sweep started before the first measurement: thrown away
    lidarBuf.erase(lidarBuf.begin());                 // (lidarBuf.clean(lidar_start_time): the keys <= the first one)
    return false;
  }
  return true;
}

void featureExtraction::laserCloudHandler(const so_wire::PointCloud2& msg) {
  frameCount = frameCount + 1;  // :712-715
  if (frameCount % config_.skipFrame != 0) return;
  so_wire::PointCloud2 copy = msg;
  manageLidarBuffer(std::move(copy), msg.header.stamp.sec + msg.header.stamp.nanosec * 1e-9);  // :761
  if (IMU_INIT == true || imuBuf.empty()) {  // :763-769
    undistortionAndFeatureExtraction();
    if (!lidarBuf.empty()) lidarBuf.erase(lidarBuf.begin());  // lidarBuf.clean(lidar_first_time)
  }
}

static std::vector<so_icp_stamped_pose> table_of(const std::map<double, so_icp_stamped_pose>& b) {
  std::vector<so_icp_stamped_pose> v;
  v.reserve(b.size());
  for (const auto& kv : b) v.push_back(kv.second);
  return v;
}

// undistortionAndFeatureExtraction (:440-499)
void featureExtraction::undistortionAndFeatureExtraction() {
  const bool imu_sync = synchronize_measurements(imuBuf);
  bool camera_sync = synchronize_measurements(visualOdomBuf);
  camera_sync = frameCount > 100 && camera_sync;  // :445-448
  if ((imu_sync || camera_sync) && !lidarBuf.empty()) {
    const double lidar_start_time = lidarBuf.begin()->first;
    const Sweep& sweep = lidarBuf.begin()->second;
    // both synchronised, or the camera only: de-skew against the VIO poses (:458-468); the IMU only: against the IMU's (:470-474)
    if (camera_sync) extractFeatures(lidar_start_time, sweep, table_of(visualOdomBuf), false, nullptr);
    else extractFeatures(lidar_start_time, sweep, table_of(imuBuf), true, nullptr);
  } else if (imuBuf.empty()) {  // :482-494: no IMU, LiDAR odometry only, identity quaternion, no de-skew
    if (lidarBuf.empty()) return;  // (the reference reads the first sweep of an empty buffer here)
    const double identity[4] = {0, 0, 0, 1};
    extractFeatures(lidarBuf.begin()->first, lidarBuf.begin()->second, {}, false, identity);
  }
  // else: "sync unsuccessfull, skipping scan frame" (:495-498)
}

// removePointDistortion (when poses are given) + extractFeatures -> uniformFeatureExtraction + publishTopic (:422-437)
bool featureExtraction::extractFeatures(double lidar_start_time, const Sweep& sweep, const std::vector<so_icp_stamped_pose>& poses, bool imu,
                                        const double q_w_original[4]) {
  so_icp_sweep_layout lay;
  if (!layout_of(sweep.msg, lay)) {
    ++frames_failed;
    last_error = "PointCloud2: data shorter than row_step * height";
    return false;
  }
  const size_t n = (size_t)sweep.msg.width * sweep.msg.height;
  nodist_.resize(n * 32);
  surf_.resize(n * 32);
  so_icp_feature_info info;
  const int rc = so_icp_extract_features(ctx_, sweep.msg.data.data(), sweep.msg.width, sweep.msg.height, &lay, lidar_start_time,
                                         poses.empty() ? nullptr : poses.data(), poses.size(), imu ? 1 : 0, config_.T_i_l,
                                         nodist_.data(), surf_.data(), &info);
  if (rc != SO_ICP_OK) {
    ++frames_failed;
    last_error = so_icp_last_error(ctx_);
    return false;
  }
  if (info.deskewed) {  // q_w_original_l / t_w_original_l = T_w_original_sensor (:289-290)
    for (int k = 0; k < 4; ++k) q_w_original_l[k] = info.q_w_original_l[k];
    for (int k = 0; k < 3; ++k) t_w_original_l[k] = info.t_w_original_l[k];
  }
  // the de-skew branches pass the member just set; the no-IMU branch an identity quaternion, with the member t_w_original_l
  // left from the sweep before (publishTopic reads it either way)
  publishTopic(lidar_start_time, sweep, info, q_w_original ? q_w_original : q_w_original_l);
  return true;
}

// pcl::toROSMsg of an unorganised cloud of 32-byte records (width = size, height = 1)
static so_wire::PointCloud2 cloud_of(const so_wire::Header& h, uint32_t width, uint32_t height, bool with_time_ring, bool is_dense,
                                     const uint8_t* data, size_t n) {
  using PF = so_wire::PointField;
  so_wire::PointCloud2 m;
  m.header = h;
  m.height = height; m.width = width;
  m.fields = {{"x", 0, PF::FLOAT32, 1}, {"y", 4, PF::FLOAT32, 1}, {"z", 8, PF::FLOAT32, 1}, {"intensity", 16, PF::FLOAT32, 1}};
  if (with_time_ring) { m.fields.push_back({"time", 20, PF::FLOAT32, 1}); m.fields.push_back({"ring", 24, PF::UINT16, 1}); }
  m.is_bigendian = false;
  m.point_step = 32; m.row_step = 32 * width;
  m.data.assign(data, data + n * 32);
  m.is_dense = is_dense;
  return m;
}

// publishTopic (:389-420) with publishCloud (:379-387)
void featureExtraction::publishTopic(double lidar_start_time, const Sweep& sweep, const so_icp_feature_info& info, const double q[4]) {
  so_wire::LaserFeature lf;
  const int64_t ns = (int64_t)(lidar_start_time * 1e9);  // rclcpp::Time(lidar_start_time*1e9): the double becomes int64 nanoseconds
  so_wire::Header h;
  h.stamp.sec = (int32_t)(ns / 1000000000); h.stamp.nanosec = (uint32_t)(ns % 1000000000);
  h.frame_id = config_.WORLD_FRAME;
  lf.header = h;
  so_wire::Header ch = h;
  ch.frame_id = config_.SENSOR_FRAME;
  // cloud_nodistortion: fromROSMsg keeps the message's width / height (velodyne); the Ouster cloud is resize()d (height 1)
  const size_t n = (size_t)sweep.msg.width * sweep.msg.height;
  const bool ouster = config_.sensor == SensorType::OUSTER;
  lf.cloud_nodistortion = cloud_of(ch, ouster ? (uint32_t)n : sweep.msg.width, ouster ? 1u : sweep.msg.height, true, sweep.msg.is_dense,
                                   nodist_.data(), n);
  const uint8_t* none = nullptr;
  lf.cloud_corner = cloud_of(ch, 0, 1, false, true, none, 0);
  lf.cloud_surface = cloud_of(ch, (uint32_t)info.n_surface, 1, false, true, surf_.data(), info.n_surface);
  lf.cloud_realsense = cloud_of(ch, 0, 1, false, true, none, 0);
  lf.initial_quaternion_x = q[0]; lf.initial_quaternion_y = q[1]; lf.initial_quaternion_z = q[2]; lf.initial_quaternion_w = q[3];
  lf.initial_pose_x = t_w_original_l[0]; lf.initial_pose_y = t_w_original_l[1]; lf.initial_pose_z = t_w_original_l[2];
  lf.imu_available = 1;  // set false, then true (:398, :417)
  lf.odom_available = 0;
  lf.sensor = 0;
  out_->publish(config_.ProjectName + "/feature_info", "super_odometry_msgs/msg/LaserFeature", so_wire::serialize(lf));
}

template bool featureExtraction::synchronize_measurements(const std::map<double, so_icp_stamped_pose>&);

}  // namespace super_odometry_soicp
