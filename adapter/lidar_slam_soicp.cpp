// lidar_slam_soicp.cpp -- see lidar_slam_soicp.h.  What LidarSLAM::Localization (src/LidarProcess/LidarSlam.cpp:30-51)
// and its read-backs become on top of the C ABI; errors travel as exceptions because that is the reference's convention
// on this path (process() catches std::exception, logs and continues: src/LaserMapping/laserMapping.cpp:788-790).
#include "lidar_slam_soicp.h"

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

namespace super_odometry_soicp {

LidarSLAM::~LidarSLAM() { if (gpu_) so_icp_destroy(gpu_); }

void LidarSLAM::ensure_context() {
  if (gpu_) return;
  so_icp_config cfg;
  so_icp_default_config(&cfg);
  cfg.device_id = device_id;
  cfg.max_iterations = (int)LocalizationICPMaxIter;             // laserMapping.cpp:108
  cfg.max_surface_features = OptSet.max_surface_features;       // :111
  cfg.velocity_failure_threshold = OptSet.velocity_failure_threshold;  // :110
  cfg.yaw_ratio = OptSet.yaw_ratio;                             // :112
  cfg.line_res = localMap.lineRes_; cfg.plane_res = localMap.planeRes_;  // :103-104
  gpu_ = so_icp_create(&cfg);
  if (!gpu_) throw std::runtime_error(std::string("so_icp_create: ") + so_icp_last_error(nullptr));
  // SOICP_NODE_MAP_INTENSITY=1: the surf cloud's intensity travels through pre-filter, map insert and map export, as in the reference's
  // PointXYZI clouds (so_icp_set_cloud_intensity); off by default: the map topics carry x y z and zeros
  const char* ev = std::getenv("SOICP_NODE_MAP_INTENSITY");
  if (ev && std::atoi(ev) && so_icp_set_cloud_intensity(gpu_, (int)offsetof(Point, intensity)) < 0)
    throw std::runtime_error(std::string("so_icp_set_cloud_intensity: ") + so_icp_last_error(gpu_));
}

void LocalMapFacade::setOrigin(const Vector3d& t) {
  owner_->ensure_context();
  const double tt[3] = {t.x(), t.y(), t.z()};
  if (so_icp_map_set_origin(*ctx_, tt, nullptr) < 0) throw std::runtime_error(so_icp_last_error(*ctx_));
}
void LocalMapFacade::addSurfPointCloud(const PointCloud<Point>& cloud) {
  owner_->ensure_context();
  if (so_icp_set_resolution(*ctx_, lineRes_, planeRes_) < 0) throw std::runtime_error(so_icp_last_error(*ctx_));
  if (cloud.points.empty()) return;
  if (so_icp_map_add_surf(*ctx_, reinterpret_cast<const float*>(cloud.points.data()), cloud.points.size(), sizeof(Point)) < 0)
    throw std::runtime_error(so_icp_last_error(*ctx_));
}
PointCloud<Point> LocalMapFacade::export_points(int only_5x5, const int pos[3]) {
  PointCloud<Point> out;
  if (!*ctx_) return out;
  size_t n = 0;
  if (so_icp_map_size(*ctx_, &n, nullptr) < 0) throw std::runtime_error(so_icp_last_error(*ctx_));
  std::vector<float> xyz(3 * (n ? n : 1));
  if (so_icp_map_export(*ctx_, xyz.data(), n, &n, only_5x5, pos) < 0) throw std::runtime_error(so_icp_last_error(*ctx_));
  out.points.resize(n);
  for (size_t i = 0; i < n; ++i) { out.points[i].x = xyz[3 * i]; out.points[i].y = xyz[3 * i + 1]; out.points[i].z = xyz[3 * i + 2]; }
  return out;
}
size_t LocalMapFacade::exportRecords(void* out, size_t cap_points, bool only_5x5, const Vector3i& p) {
  if (!*ctx_) return 0;
  const int pos[3] = {p.x(), p.y(), p.z()};
  size_t n = 0;
  if (so_icp_map_export_records(*ctx_, out, sizeof(Point), cap_points, &n, only_5x5 ? 1 : 0, pos) < 0) throw std::runtime_error(so_icp_last_error(*ctx_));
  return n;
}
PointCloud<Point> LocalMapFacade::get5x5LocalMap(const Vector3i& p) { const int pos[3] = {p.x(), p.y(), p.z()}; return export_points(1, pos); }
PointCloud<Point> LocalMapFacade::getAllLocalMap() { const int pos[3] = {0, 0, 0}; return export_points(0, pos); }

void LidarSLAM::StageNextScan(const PointCloud<Point>::Ptr& planner_point) {
  ensure_context();
  if (!planner_point || planner_point->points.empty()) return;
  if (so_icp_stage_scan(gpu_, reinterpret_cast<const float*>(planner_point->points.data()), planner_point->points.size(), sizeof(Point)) < 0)
    throw std::runtime_error(so_icp_last_error(gpu_));
}

void LidarSLAM::push_knobs() {
  // knobs the node writes into public fields before every call (laserMapping.cpp:648-649, 703-711)
  if (so_icp_set_resolution(gpu_, localMap.lineRes_, localMap.planeRes_) < 0) throw std::runtime_error(so_icp_last_error(gpu_));
  so_icp_set_max_surface_features(gpu_, OptSet.max_surface_features);
  so_icp_set_max_iterations(gpu_, (int)LocalizationICPMaxIter);
  if (keep_correspondences != pushed_keep_correspondences_) {
    if (so_icp_keep_correspondences(gpu_, keep_correspondences ? 1 : 0) < 0) throw std::runtime_error(so_icp_last_error(gpu_));
    pushed_keep_correspondences_ = keep_correspondences;
    if (!keep_correspondences) pushed_keep_correspondence_geometry_ = false;  // (the library turns the geometry switch off with it)
  }
  const bool geometry = keep_correspondences && keep_correspondence_geometry;
  if (geometry != pushed_keep_correspondence_geometry_) {
    if (so_icp_keep_correspondence_geometry(gpu_, geometry ? 1 : 0) < 0) throw std::runtime_error(so_icp_last_error(gpu_));
    pushed_keep_correspondence_geometry_ = geometry;
  }
}

int LidarSLAM::LastCorrespondenceGeometry(std::vector<so_icp_correspondence_geometry_record>& out, so_icp_correspondence_geometry_info* info) {
  ensure_context();
  so_icp_correspondence_geometry_info local;
  if (!info) info = &local;
  const size_t cap = last_raw.n_iterations > 0 && last_raw.n_iterations <= SO_ICP_MAX_OUTER ? (size_t)last_raw.iterations[last_raw.n_iterations - 1].num_surf_from_scan : 0;
  out.resize(cap);
  if (so_icp_correspondence_geometry(gpu_, out.data(), out.size(), nullptr, 0, nullptr, info) < 0)
    throw std::runtime_error(std::string("so_icp_correspondence_geometry: ") + so_icp_last_error(gpu_));
  if (info->n_accepted > out.size()) {  // (a set the adapter's own statistics do not describe: sized by the call's answer)
    out.resize((size_t)info->n_accepted);
    if (so_icp_correspondence_geometry(gpu_, out.data(), out.size(), nullptr, 0, nullptr, info) < 0)
      throw std::runtime_error(std::string("so_icp_correspondence_geometry: ") + so_icp_last_error(gpu_));
  }
  out.resize((size_t)info->n_accepted);
  return (int)info->n_accepted;
}

int LidarSLAM::LastCorrespondences(const Transformd* pose, std::vector<so_icp_correspondence>& out, so_icp_correspondence_info* info) {
  ensure_context();
  so_icp_correspondence_info local;
  if (!info) info = &local;
  double T[7];
  if (pose) { T[0] = pose->pos.x(); T[1] = pose->pos.y(); T[2] = pose->pos.z(); T[3] = pose->rot.x(); T[4] = pose->rot.y(); T[5] = pose->rot.z(); T[6] = pose->rot.w(); }
  // the registration counted the accepted points (iterations.back().num_surf_from_scan): room for them, one call
  const size_t cap = last_raw.n_iterations > 0 && last_raw.n_iterations <= SO_ICP_MAX_OUTER ? (size_t)last_raw.iterations[last_raw.n_iterations - 1].num_surf_from_scan : 0;
  out.resize(cap);
  if (so_icp_correspondences(gpu_, pose ? T : nullptr, out.data(), out.size(), nullptr, nullptr, 0, nullptr, info) < 0)
    throw std::runtime_error(std::string("so_icp_correspondences: ") + so_icp_last_error(gpu_));
  if (info->n_accepted > out.size()) {  // (a set the adapter's own statistics do not describe: sized by the call's answer)
    out.resize((size_t)info->n_accepted);
    if (so_icp_correspondences(gpu_, pose ? T : nullptr, out.data(), out.size(), nullptr, nullptr, 0, nullptr, info) < 0)
      throw std::runtime_error(std::string("so_icp_correspondences: ") + so_icp_last_error(gpu_));
  }
  out.resize((size_t)info->n_accepted);
  return (int)info->n_accepted;
}

int LidarSLAM::MatchPlanes(const Transformd& T, const PointCloud<Point>::Ptr& planner_point, so_icp_stats* st) {
  ensure_context();
  push_knobs();
  const double pose[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
  const float* xyz = planner_point && !planner_point->points.empty() ? reinterpret_cast<const float*>(planner_point->points.data()) : nullptr;
  const size_t n = planner_point ? planner_point->points.size() : 0;
  const int rc = so_icp_match(gpu_, xyz, n, sizeof(Point), pose, st);
  if (rc < 0) throw std::runtime_error(std::string("so_icp_match: ") + so_icp_last_error(gpu_));
  return rc;
}

void LidarSLAM::CorrespondenceSums(const std::vector<Transformd>& poses, std::vector<so_icp_sums>& sums) {
  ensure_context();
  std::vector<double> flat(poses.size() * 7);
  for (size_t k = 0; k < poses.size(); ++k) {
    const Transformd& T = poses[k];
    const double p[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
    std::copy(p, p + 7, flat.begin() + 7 * k);
  }
  sums.resize(poses.size());
  if (so_icp_correspondence_sums(gpu_, flat.data(), (int)poses.size(), sums.data()) < 0)
    throw std::runtime_error(std::string("so_icp_correspondence_sums: ") + so_icp_last_error(gpu_));
}

void LidarSLAM::read_back(int32_t n_edge_points, const double T_out[7], double timeLaserOdometry) {
  const so_icp_stats& st = last_raw;
  last_flags = st.flags;
  T_w_lidar.pos = Vector3d(T_out[0], T_out[1], T_out[2]);                 // read back at laserMapping.cpp:734-737
  T_w_lidar.rot = Quaterniond(T_out[6], T_out[3], T_out[4], T_out[5]);
  last_T_w_lidar = T_w_lidar;                                            // LidarSlam.cpp:197
  lasttimeLaserOdometry = timeLaserOdometry;
  if (last_status == SO_ICP_MAP_SEEDED) return;  // initialization == false (LidarSlam.cpp:45-46): initializeMapping only
  // from here on the call went through EstimateLidarUncertainty (:47) and prepareOptimizationState (:361-377)
  pos_in_localmap = Vector3i(st.pos_in_localmap[0], st.pos_in_localmap[1], st.pos_in_localmap[2]);  // :363, read at laserMapping.cpp:439
  stats.laser_cloud_surf_from_map_num = st.laser_cloud_surf_from_map_num;
  stats.laser_cloud_surf_stack_num = st.laser_cloud_surf_stack_num;
  stats.laser_cloud_corner_from_map_num = 0;                  // no corner map exists: nothing calls addEdgePointCloud
  stats.laser_cloud_corner_stack_num = n_edge_points;         // EdgesPoints->size(), LidarSlam.cpp:374
  stats.uncertainty_x = st.uncertainty[0]; stats.uncertainty_y = st.uncertainty[1]; stats.uncertainty_z = st.uncertainty[2];
  stats.uncertainty_roll = st.uncertainty[3]; stats.uncertainty_pitch = st.uncertainty[4]; stats.uncertainty_yaw = st.uncertainty[5];
  stats.iterations.clear();                                   // updateFeatureStats, :376
  if (last_status != SO_ICP_OK) return;  // "Not enough features for optimization" (:113-116): the rest of the statistics keeps its values
  startupCount = st.startup_count;                                       // laserMapping.cpp:738
  // OptimizationStats message (laserMapping.cpp:581-596; LidarSlam.cpp:198-210, 242-251, 969-974)
  stats.total_translation = st.total_translation; stats.total_rotation = st.total_rotation;
  stats.translation_from_last = st.translation_from_last; stats.rotation_from_last = st.rotation_from_last;
  stats.time_elapsed = st.time_elapsed_ms;
  stats.prediction_source = st.prediction_source;                         // LidarSlam.cpp:278, 297
  for (int i = 0; i < st.n_iterations; ++i) {
    IterationStats it;
    it.translation_norm = st.iterations[i].translation_norm; it.rotation_norm = st.iterations[i].rotation_norm;
    it.num_surf_from_scan = st.iterations[i].num_surf_from_scan; it.num_corner_from_scan = 0;
    stats.iterations.push_back(it);
  }
}

void LidarSLAM::SetPosePrior(const Transformd& T, const double information[36]) {
  ensure_context();
  const double T_meas[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
  so_icp_pose_prior prior;
  if (so_icp_pose_prior_from_information(information, T_meas, &prior) != SO_ICP_OK)
    throw std::invalid_argument("SetPosePrior: the information matrix is not positive semi-definite");
  if (so_icp_set_pose_prior(gpu_, &prior) < 0) throw std::runtime_error(std::string("so_icp_set_pose_prior: ") + so_icp_last_error(gpu_));
}

void LidarSLAM::SetSequencePriors(const std::vector<so_icp_pose_prior>& priors, const std::vector<uint8_t>& modes) {
  ensure_context();
  if (!modes.empty() && modes.size() != priors.size()) throw std::invalid_argument("SetSequencePriors: one mode per prior");
  if (so_icp_set_sequence_priors(gpu_, (int)priors.size(), priors.empty() ? nullptr : priors.data(), modes.empty() ? nullptr : modes.data()) < 0)
    throw std::runtime_error(std::string("so_icp_set_sequence_priors: ") + so_icp_last_error(gpu_));
}

// shouldAddAbsolutePoseConstraints + addAbsolutePoseConstraints, LidarSlam.cpp:281-297: information = diag((1 - uncertainty_xyz) *
// max(50, int(n * 0.1)) * V, max(10, int(n * 0.01)) * V twice, max(5, int(n * 0.001)) * 0) on `position`, n the feature count of every
// evaluation -- stated exactly by U = its square root without the counts, and the counts as the rows' floor and fraction.  The
// uncertainties are those this object holds, from the frame before (lidarOdomUncer).
void LidarSLAM::add_absolute_pose_constraints(bool initialization, PredictionSource predictodom, const Transformd& position) {
  if (!initialization || !(predictodom == PredictionSource::VIO_ODOM && isDegenerate == true && Visual_confidence_factor != 0)) return;
  so_icp_pose_prior prior;
  std::memset(&prior, 0, sizeof(prior));
  const double T_meas[7] = {position.pos.x(), position.pos.y(), position.pos.z(), position.rot.x(), position.rot.y(), position.rot.z(), position.rot.w()};
  std::memcpy(prior.T_meas, T_meas, sizeof(T_meas));
  const double V = Visual_confidence_factor;
  const double diag[6] = {std::sqrt((1 - stats.uncertainty_x) * V), std::sqrt((1 - stats.uncertainty_y) * V), std::sqrt((1 - stats.uncertainty_z) * V),
                          std::sqrt(V), std::sqrt(V), 0.0};
  const double floor_[6] = {50, 50, 50, 10, 10, 5}, fraction[6] = {0.1, 0.1, 0.1, 0.01, 0.01, 0.001};
  for (int i = 0; i < 6; ++i) { prior.sqrt_information[7 * i] = diag[i]; prior.count_floor[i] = floor_[i]; prior.count_fraction[i] = fraction[i]; }
  if (so_icp_set_pose_prior(gpu_, &prior) < 0) throw std::runtime_error(std::string("so_icp_set_pose_prior: ") + so_icp_last_error(gpu_));
}

void LidarSLAM::Localization(bool initialization, PredictionSource predictodom /*read by the VIO prior alone, LidarSlam.cpp:281-283*/,
                             Transformd position, PointCloud<Point>::Ptr edge_point /*dead path, LidarSlam.cpp:402-512: only its size is reported*/,
                             PointCloud<Point>::Ptr planner_point, double timeLaserOdometry) {
  ensure_context();
  push_knobs();
  const double T_in[7] = {position.pos.x(), position.pos.y(), position.pos.z(),
                          position.rot.x(), position.rot.y(), position.rot.z(), position.rot.w()};
  double T_out[7];
  const float* xyz = planner_point && !planner_point->points.empty() ? reinterpret_cast<const float*>(planner_point->points.data()) : nullptr;
  const size_t n = planner_point ? planner_point->points.size() : 0;
  add_absolute_pose_constraints(initialization, predictodom, position);
  last_status = so_icp_localization(gpu_, initialization ? 1 : 0, T_in, xyz, n, sizeof(Point), timeLaserOdometry, T_out, &last_raw);
  if (last_status < 0) throw std::runtime_error(std::string("so_icp_localization: ") + so_icp_last_error(gpu_));
  read_back(edge_point ? (int32_t)edge_point->points.size() : 0, T_out, timeLaserOdometry);
}

int LidarSLAM::LocalizationSequence(Transformd position, const std::vector<PointCloud<Point>::Ptr>& planner_points,
                                    const std::vector<Transformd>& predictions, const std::vector<double>& times,
                                    std::vector<Transformd>* poses_out, std::vector<so_icp_stats>* stats_out) {
  const size_t count = planner_points.size();
  if (predictions.size() != count || times.size() != count) throw std::invalid_argument("LocalizationSequence: one prediction and one stamp per cloud");
  ensure_context();
  push_knobs();
  if (count == 0) return 0;
  auto to7 = [](const Transformd& T, double* o) {
    o[0] = T.pos.x(); o[1] = T.pos.y(); o[2] = T.pos.z(); o[3] = T.rot.x(); o[4] = T.rot.y(); o[5] = T.rot.z(); o[6] = T.rot.w();
  };
  std::vector<const void*> scans(count);
  std::vector<size_t> n(count);
  std::vector<double> deltas(7 * count), poses(7 * count);
  std::vector<so_icp_stats> st(count);
  for (size_t k = 0; k < count; ++k) {
    const PointCloud<Point>* cl = planner_points[k].get();
    n[k] = cl ? cl->points.size() : 0;
    scans[k] = n[k] ? static_cast<const void*>(cl->points.data()) : nullptr;
    to7(predictions[k], &deltas[7 * k]);
  }
  double T_in[7];
  to7(position, T_in);
  int n_done = 0;
  last_status = so_icp_localization_sequence(gpu_, (int)count, scans.data(), n.data(), sizeof(Point), 0, T_in, deltas.data(), times.data(),
                                             poses.data(), nullptr, st.data(), &n_done);
  if (last_status < 0) throw std::runtime_error(std::string("so_icp_localization_sequence: ") + so_icp_last_error(gpu_));
  if (poses_out) {
    poses_out->clear();
    for (int k = 0; k < n_done; ++k) {
      Transformd T;
      T.pos = Vector3d(poses[7 * k], poses[7 * k + 1], poses[7 * k + 2]);
      T.rot = Quaterniond(poses[7 * k + 6], poses[7 * k + 3], poses[7 * k + 4], poses[7 * k + 5]);
      poses_out->push_back(T);
    }
  }
  if (stats_out) stats_out->assign(st.begin(), st.begin() + n_done);
  // the public fields: those of the last frame the run reached (the one that stopped it, if any)
  // (a frame stopped by SO_ICP_NOT_ENOUGH_MAP_FEATURES reports its guess as its pose, like so_icp_localization)
  const size_t last = std::min((size_t)n_done, count - 1);
  last_raw = st[last];
  read_back(0, &poses[7 * last], times[last]);
  return n_done;
}

void LidarSLAM::AnnounceSurf(const float* xyz, size_t n, size_t stride_bytes) {
  if (gpu_ && xyz && n) (void)so_icp_prefilter_announce(gpu_, xyz, n, stride_bytes);  // (a refused announcement only means "not staged ahead")
}

void LidarSLAM::PrefilterSurf(const float* xyz, size_t n, size_t stride_bytes, bool auto_voxel_size, float line_res, float plane_res,
                              so_icp_prefilter_info* info, const void** d_filtered, size_t* n_filtered) {
  ensure_context();
  void* d = nullptr;
  const int rc = so_icp_prefilter_scan(gpu_, xyz, n, stride_bytes, auto_voxel_size ? 1 : 0, line_res, plane_res, &d, n_filtered, info);
  if (rc < 0) throw std::runtime_error(std::string("so_icp_prefilter_scan: ") + so_icp_last_error(gpu_));
  *d_filtered = d;
  if (info) { localMap.lineRes_ = info->line_res; localMap.planeRes_ = info->plane_res; }  // laserMapping.cpp:648-649
}

size_t LidarSLAM::TransformCloud(void* points, size_t n, size_t stride_bytes, const Transformd& T, std::vector<uint8_t>& keep) {
  ensure_context();
  const double Tw[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
  keep.resize(n);
  size_t kept = 0;
  if (so_icp_transform_cloud(gpu_, points, n, stride_bytes, Tw, keep.data(), &kept) < 0)
    throw std::runtime_error(std::string("so_icp_transform_cloud: ") + so_icp_last_error(gpu_));
  return kept;
}

size_t LidarSLAM::RegisteredScan(const void* records, size_t n, size_t stride_bytes, const Transformd& T, void* out) {
  ensure_context();
  const double Tw[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
  size_t kept = 0;
  if (so_icp_registered_scan(gpu_, records, n, stride_bytes, Tw, out, &kept) < 0)
    throw std::runtime_error(std::string("so_icp_registered_scan: ") + so_icp_last_error(gpu_));
  return kept;
}

uint8_t* LidarSLAM::PinnedScratch(int which, size_t bytes) {
  ensure_context();
  if ((size_t)which >= scratch_.size()) scratch_.resize((size_t)which + 1);
  Scratch& sc = scratch_[(size_t)which];
  if (sc.cap < bytes) {
    if (sc.p) so_icp_host_free(gpu_, sc.p);
    sc.p = nullptr; sc.cap = 0;
    void* p = nullptr;
    const size_t want = bytes + bytes / 4 + 4096;
    if (so_icp_host_alloc(gpu_, want, &p) < 0) throw std::runtime_error(std::string("so_icp_host_alloc: ") + so_icp_last_error(gpu_));
    sc.p = static_cast<uint8_t*>(p); sc.cap = want;
  }
  return sc.p;
}

void LidarSLAM::LocalizationPrefiltered(bool initialization, PredictionSource predictodom, Transformd position, const void* d_planner_xyz, size_t n_planner,
                                        int32_t n_edge_points, double timeLaserOdometry) {
  ensure_context();
  push_knobs();
  const double T_in[7] = {position.pos.x(), position.pos.y(), position.pos.z(),
                          position.rot.x(), position.rot.y(), position.rot.z(), position.rot.w()};
  double T_out[7];
  add_absolute_pose_constraints(initialization, predictodom, position);
  last_status = so_icp_localization_dev(gpu_, initialization ? 1 : 0, T_in, d_planner_xyz, n_planner, timeLaserOdometry, T_out, &last_raw);
  if (last_status < 0) throw std::runtime_error(std::string("so_icp_localization_dev: ") + so_icp_last_error(gpu_));
  read_back(n_edge_points, T_out, timeLaserOdometry);
}

}  // namespace super_odometry_soicp
