// adapter_driver.cpp -- C++ caller of the boundary (test binary, built by __graft_entry__.build(), run by a -m gpu test):
// drives the adapter exactly like laserMapping::performSLAMOptimization does (src/LaserMapping/laserMapping.cpp:703-741):
// first frame with initialization == false (map seeding), then Localization() per frame, reading back the public fields.
//
//   adapter_driver <in.bin> <out.bin> [--sequence]
// in.bin : int32 n_frames, float32 plane_res, int32 max_iterations, int32 max_surface_features; per frame: int32 n,
//          float64 guess[7], float64 time, float32 xyz[n][3]  (sensor frame, as the node passes it)
// out.bin: per frame: int32 status, int32 startupCount, int32 pos_in_localmap[3], float64 T_w_lidar[7] (tx ty tz qx qy qz qw),
//          int32 n_iterations, int32 surf_from_map, float64 total_translation, float64 uncertainty[6],
//          int32 num_surf of the last iteration, uint32 flags;  then: uint64 map size, float32 map xyz (5x5 neighbourhood)
// --sequence: a replay (LidarSLAM::LocalizationSequence): frame 0 seeds the map, frames 1.. run as ONE sequence from guess 1 with the
//          motion predictions guess_(k-1)^-1 * guess_k; prints one line per frame (index and pose, %.17g) and writes
//          out.bin: int32 status, int32 n_done, float64 T_w_lidar[n_done][7]
//          --sequence --prior-at-guess: every frame of the run carries an absolute pose prior measured at its own guess
//          (LidarSLAM::SetSequencePriors, SO_ICP_PRIOR_AT_GUESS): the U of --vio-prior with the uncertainty terms at 0
// --correspondences: the frames as without a flag, with LidarSLAM::keep_correspondences on; behind the output above, the last frame's
//          correspondence set (LidarSLAM::LastCorrespondences at the optimised pose): the so_icp_correspondence_info as it is, then
//          n_accepted so_icp_correspondence records as they are
// --seam-c: the frames as without a flag, but every frame after the seeding one is registered by the HOST loop below (the reference's
//          LidarSlam.cpp:119-148 around LidarSLAM::MatchPlanes, LidarSLAM::CorrespondenceSums and so_icp_lm_begin / _feed: what a caller
//          that keeps its own solver writes) instead of Localization()'s registration, and its scan inserted at that pose through
//          localMap.addSurfPointCloud.  Same output format; the fields a registration derives from the tracker (startupCount,
//          uncertainty) stay as the match reports them, total_translation is |pose - guess|, flags those of the last match
// --vio-prior: the frames as without a flag, with predictodom = VIO_ODOM, isDegenerate set and Visual_confidence_factor = 0.9 on every frame:
//          Localization() adds the reference's absolute pose prior on the guess (LidarSlam.cpp:281-297).  Same output; one line per frame
//          on stdout: index, stats.prediction_source
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "lidar_slam_soicp.h"

using namespace super_odometry_soicp;

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }
template <typename T> static void wr(FILE* f, const T& v) { fwrite(&v, sizeof(T), 1, f); }

// a^-1 * b (Twist.h:172-185): the motion prediction that takes pose a to pose b, in a's frame
static Transformd between(const Transformd& a, const Transformd& b) {
  const Quaterniond& q = a.rot;
  const double ax = -q.x(), ay = -q.y(), az = -q.z(), aw = q.w();  // conj(q)
  const double vx = b.pos.x() - a.pos.x(), vy = b.pos.y() - a.pos.y(), vz = b.pos.z() - a.pos.z();
  // t = conj(q) v conj(q)^-1 = v + 2 w (u x v) + 2 u x (u x v), u = (ax, ay, az)
  const double cx = ay * vz - az * vy, cy = az * vx - ax * vz, cz = ax * vy - ay * vx;
  const double tx = vx + 2 * (aw * cx + ay * cz - az * cy), ty = vy + 2 * (aw * cy + az * cx - ax * cz), tz = vz + 2 * (aw * cz + ax * cy - ay * cx);
  const Quaterniond& r = b.rot;
  const double w = aw * r.w() - ax * r.x() - ay * r.y() - az * r.z();
  const double x = aw * r.x() + ax * r.w() + ay * r.z() - az * r.y();
  const double y = aw * r.y() - ax * r.z() + ay * r.w() + az * r.x();
  const double z = aw * r.z() + ax * r.y() - ay * r.x() + az * r.w();
  Transformd d;
  d.pos = Vector3d(tx, ty, tz); d.rot = Quaterniond(w, x, y, z);
  return d;
}

// LidarSlam.cpp:119-148 on the host: match at the current pose; so_icp_lm_begin on the match's sums; one CorrespondenceSums per
// candidate -> so_icp_lm_feed until the solver is done; stop at num_successful_steps == 1 or the last iteration.  Returns the match's
// code when a match did not end with SO_ICP_OK.  *st: the statistics of the last match; *n_outer: outer iterations run.
static int register_through_seam(LidarSLAM& slam, const PointCloud<Point>::Ptr& cloud, Transformd& T, int max_outer, int lm_max, so_icp_stats* st,
                                 int* n_outer) {
  *n_outer = 0;
  for (int it = 0; it < max_outer; ++it) {
    const int rc = slam.MatchPlanes(T, cloud, st);
    if (rc != SO_ICP_OK) return rc;
    so_icp_sums at;
    std::memset(&at, 0, sizeof(at));
    const so_icp_iter_stats& m = st->iterations[0];
    at.cost = m.initial_cost; at.count = (double)m.num_surf_from_scan;
    for (int i = 0, k = 0; i < 6; ++i) { at.Jtr[i] = st->Jtr[i]; for (int j = i; j < 6; ++j) at.JtJ[k++] = st->JtJ[6 * i + j]; }
    for (int h = 0; h < SO_ICP_N_REJECT; ++h) at.hist[h] = (double)m.reject_hist[h];
    for (int h = 0; h < SO_ICP_N_OBS; ++h) at.hist[SO_ICP_N_REJECT + h] = (double)m.obs_hist[h];
    const double x0[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
    so_icp_lm_state S;
    double next[7];
    int more = so_icp_lm_begin(&S, x0, &at, lm_max, next);
    std::vector<Transformd> cand(1);
    std::vector<so_icp_sums> sums;
    while (more > 0) {
      cand[0].pos = Vector3d(next[0], next[1], next[2]); cand[0].rot = Quaterniond(next[6], next[3], next[4], next[5]);
      slam.CorrespondenceSums(cand, sums);
      more = so_icp_lm_feed(&S, &sums[0], next);
    }
    double x[7];
    so_icp_iter_stats solved;
    so_icp_lm_result(&S, x, &solved);
    T.pos = Vector3d(x[0], x[1], x[2]); T.rot = Quaterniond(x[6], x[3], x[4], x[5]);
    *n_outer = it + 1;
    if (solved.num_successful_steps == 1) break;
  }
  return SO_ICP_OK;
}

// TransformPoint (superodom_utils.h:119-123): rot * p + pos in double, rounded to float -- the cloud transformAndAddToMap inserts
static PointCloud<Point> to_world(const PointCloud<Point>& cloud, const Transformd& T) {
  PointCloud<Point> w = cloud;
  const double qx = T.rot.x(), qy = T.rot.y(), qz = T.rot.z(), qw = T.rot.w();
  for (Point& p : w.points) {  // Eigen::QuaternionBase::_transformVector: v + w uv + u x uv, uv = 2 (u x v)
    const double vx = p.x, vy = p.y, vz = p.z;
    double ux = qy * vz - qz * vy, uy = qz * vx - qx * vz, uz = qx * vy - qy * vx;
    ux += ux; uy += uy; uz += uz;
    p.x = (float)(vx + qw * ux + (qy * uz - qz * uy) + T.pos.x());
    p.y = (float)(vy + qw * uy + (qz * ux - qx * uz) + T.pos.y());
    p.z = (float)(vz + qw * uz + (qx * uy - qy * ux) + T.pos.z());
  }
  return w;
}

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  try {
    FILE* in = fopen(argv[1], "rb");
    FILE* out = fopen(argv[2], "wb");
    if (!in || !out) throw std::runtime_error("cannot open files");
    const int n_frames = rd<int32_t>(in);
    LidarSLAM slam;
    slam.localMap.planeRes_ = rd<float>(in);                    // laserMapping.cpp:103-104
    slam.localMap.lineRes_ = slam.localMap.planeRes_ / 2;
    slam.LocalizationICPMaxIter = (size_t)rd<int32_t>(in);      // :108
    slam.OptSet.max_surface_features = rd<int32_t>(in);         // :111
    std::vector<PointCloud<Point>::Ptr> clouds;
    std::vector<Transformd> guesses;
    std::vector<double> times;
    for (int f = 0; f < n_frames; ++f) {
      const int n = rd<int32_t>(in);
      double g[7];
      for (double& v : g) v = rd<double>(in);
      times.push_back(rd<double>(in));
      auto cloud = std::make_shared<PointCloud<Point>>();
      cloud->points.resize(n);
      for (int i = 0; i < n; ++i) { cloud->points[i].x = rd<float>(in); cloud->points[i].y = rd<float>(in); cloud->points[i].z = rd<float>(in); cloud->points[i].intensity = (float)i; }
      clouds.push_back(cloud);
      Transformd T;
      T.pos = Vector3d(g[0], g[1], g[2]); T.rot = Quaterniond(g[6], g[3], g[4], g[5]);
      guesses.push_back(T);
    }
    auto edge = std::make_shared<PointCloud<Point>>();  // dead path: the node still passes it
    if (argc > 3 && std::strcmp(argv[3], "--sequence") == 0) {
      if (n_frames < 2) throw std::runtime_error("--sequence needs at least two frames");
      slam.Localization(false, LidarSLAM::PredictionSource::LIO_ODOM, guesses[0], edge, clouds[0], times[0]);  // seeds the map
      std::vector<PointCloud<Point>::Ptr> run(clouds.begin() + 1, clouds.end());
      std::vector<double> run_times(times.begin() + 1, times.end());
      std::vector<Transformd> predictions(run.size());
      for (size_t k = 1; k < run.size(); ++k) predictions[k] = between(guesses[k], guesses[k + 1]);
      if (argc > 4 && std::strcmp(argv[4], "--prior-at-guess") == 0) {
        so_icp_pose_prior prior;
        std::memset(&prior, 0, sizeof(prior));
        prior.T_meas[6] = 1.0;  // (not read: the measurement is the frame's guess)
        const double V = 0.9, diag[6] = {std::sqrt(V), std::sqrt(V), std::sqrt(V), std::sqrt(V), std::sqrt(V), 0.0};
        const double floor_[6] = {50, 50, 50, 10, 10, 5}, fraction[6] = {0.1, 0.1, 0.1, 0.01, 0.01, 0.001};
        for (int i = 0; i < 6; ++i) { prior.sqrt_information[7 * i] = diag[i]; prior.count_floor[i] = floor_[i]; prior.count_fraction[i] = fraction[i]; }
        slam.SetSequencePriors(std::vector<so_icp_pose_prior>(run.size(), prior), std::vector<uint8_t>(run.size(), (uint8_t)SO_ICP_PRIOR_AT_GUESS));
      }
      std::vector<Transformd> poses;
      const int n_done = slam.LocalizationSequence(guesses[1], run, predictions, run_times, &poses);
      wr<int32_t>(out, slam.last_status); wr<int32_t>(out, n_done);
      for (int k = 0; k < n_done; ++k) {
        const Transformd& T = poses[(size_t)k];
        const double p[7] = {T.pos.x(), T.pos.y(), T.pos.z(), T.rot.x(), T.rot.y(), T.rot.z(), T.rot.w()};
        for (double v : p) wr<double>(out, v);
        printf("frame %d: %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", k + 1, p[0], p[1], p[2], p[3], p[4], p[5], p[6]);
      }
      printf("status %d, %d of %d frames registered and inserted, map %zu points\n", slam.last_status, n_done, (int)run.size(),
             slam.localMap.getAllLocalMap().points.size());
      fclose(in); fclose(out);
      return 0;
    }
    const bool correspondences = argc > 3 && std::strcmp(argv[3], "--correspondences") == 0;
    const bool seam_c = argc > 3 && std::strcmp(argv[3], "--seam-c") == 0;
    const bool vio_prior = argc > 3 && std::strcmp(argv[3], "--vio-prior") == 0;
    // --geometry: per registration, the number of accepted correspondences and the observability histogram summed on the device from the
    // geometry records' labels, next to the one in the registration's statistics (so_icp_correspondence_geometry)
    const bool geometry = argc > 3 && std::strcmp(argv[3], "--geometry") == 0;
    slam.keep_correspondences = correspondences || seam_c || geometry;
    slam.keep_correspondence_geometry = geometry;
    if (vio_prior) { slam.isDegenerate = true; slam.Visual_confidence_factor = 0.9; }
    bool initialization = false;                        // laserMapping.cpp: first frame seeds the map
    for (int f = 0; f < n_frames; ++f) {
      if (seam_c && initialization) {
        Transformd T = guesses[f];
        so_icp_stats st;
        int n_outer = 0;
        slam.last_status = register_through_seam(slam, clouds[f], T, (int)slam.LocalizationICPMaxIter, 4, &st, &n_outer);
        slam.last_flags = st.flags; slam.last_raw = st;
        slam.pos_in_localmap = Vector3i(st.pos_in_localmap[0], st.pos_in_localmap[1], st.pos_in_localmap[2]);
        slam.stats.laser_cloud_surf_from_map_num = st.laser_cloud_surf_from_map_num;
        slam.stats.uncertainty_x = st.uncertainty[0]; slam.stats.uncertainty_y = st.uncertainty[1]; slam.stats.uncertainty_z = st.uncertainty[2];
        slam.stats.uncertainty_roll = st.uncertainty[3]; slam.stats.uncertainty_pitch = st.uncertainty[4]; slam.stats.uncertainty_yaw = st.uncertainty[5];
        slam.stats.iterations.clear();
        if (slam.last_status == SO_ICP_OK) {
          slam.T_w_lidar = slam.last_T_w_lidar = T;
          const double dx = T.pos.x() - guesses[f].pos.x(), dy = T.pos.y() - guesses[f].pos.y(), dz = T.pos.z() - guesses[f].pos.z();
          slam.stats.total_translation = std::sqrt(dx * dx + dy * dy + dz * dz);
          for (int i = 0; i < n_outer; ++i) { IterationStats is{}; is.num_surf_from_scan = st.iterations[0].num_surf_from_scan; slam.stats.iterations.push_back(is); }
          slam.localMap.addSurfPointCloud(to_world(*clouds[f], T));  // transformAndAddToMap, LidarSlam.cpp:60-80
        }
      } else {
        if (f + 1 < n_frames && f >= 1 && !seam_c) slam.StageNextScan(clouds[f + 1]);  // what the feature callback would do
        slam.Localization(initialization, vio_prior ? LidarSLAM::PredictionSource::VIO_ODOM : LidarSLAM::PredictionSource::LIO_ODOM, guesses[f], edge, clouds[f],
                          times[f]);
        if (vio_prior) printf("frame %d: prediction_source %d\n", f, (int)slam.stats.prediction_source);
      }
      if (geometry && initialization && slam.last_status == SO_ICP_OK) {
        std::vector<so_icp_correspondence_geometry_record> recs;
        so_icp_correspondence_geometry_info info;
        slam.LastCorrespondenceGeometry(recs, &info);
        const so_icp_stats& st = slam.last_raw;
        const int32_t* sh = st.iterations[st.n_iterations > 0 ? st.n_iterations - 1 : 0].obs_hist;
        printf("frame %d: geometry valid %d n_accepted %llu records %zu obs_hist", f, (int)info.valid, (unsigned long long)info.n_accepted, recs.size());
        for (int h = 0; h < SO_ICP_N_OBS; ++h) printf(" %d", (int)info.obs_hist[h]);
        printf(" | stats");
        for (int h = 0; h < SO_ICP_N_OBS; ++h) printf(" %d", (int)sh[h]);
        printf("\n");
      }
      initialization = true;
      slam.frame_count = f; slam.laser_imu_sync = 1;    // :740-741
      wr<int32_t>(out, slam.last_status); wr<int32_t>(out, slam.startupCount);
      wr<int32_t>(out, slam.pos_in_localmap.x()); wr<int32_t>(out, slam.pos_in_localmap.y()); wr<int32_t>(out, slam.pos_in_localmap.z());
      wr<double>(out, slam.T_w_lidar.pos.x()); wr<double>(out, slam.T_w_lidar.pos.y()); wr<double>(out, slam.T_w_lidar.pos.z());
      wr<double>(out, slam.T_w_lidar.rot.x()); wr<double>(out, slam.T_w_lidar.rot.y()); wr<double>(out, slam.T_w_lidar.rot.z()); wr<double>(out, slam.T_w_lidar.rot.w());
      wr<int32_t>(out, (int32_t)slam.stats.iterations.size()); wr<int32_t>(out, slam.stats.laser_cloud_surf_from_map_num);
      wr<double>(out, slam.stats.total_translation);
      wr<double>(out, slam.stats.uncertainty_x); wr<double>(out, slam.stats.uncertainty_y); wr<double>(out, slam.stats.uncertainty_z);
      wr<double>(out, slam.stats.uncertainty_roll); wr<double>(out, slam.stats.uncertainty_pitch); wr<double>(out, slam.stats.uncertainty_yaw);
      wr<int32_t>(out, slam.stats.iterations.empty() ? 0 : slam.stats.iterations.back().num_surf_from_scan);
      wr<uint32_t>(out, slam.last_flags);
      // the node pads / clears the iteration list after publishing (laserMapping.cpp:588-596)
      slam.stats.iterations.clear();
    }
    const PointCloud<Point> near = slam.localMap.get5x5LocalMap(slam.pos_in_localmap);  // laserMapping.cpp:439
    wr<uint64_t>(out, (uint64_t)near.points.size());
    for (const Point& p : near.points) { wr<float>(out, p.x); wr<float>(out, p.y); wr<float>(out, p.z); }
    if (correspondences) {
      std::vector<so_icp_correspondence> recs;
      so_icp_correspondence_info info;
      slam.LastCorrespondences(nullptr, recs, &info);
      wr(out, info);
      if (!recs.empty()) fwrite(recs.data(), sizeof(so_icp_correspondence), recs.size(), out);
    }
    fclose(in); fclose(out);
  } catch (const std::exception& e) {
    fprintf(stderr, "adapter_driver: %s\n", e.what());  // what process() would log (laserMapping.cpp:788-790)
    return 1;
  }
  return 0;
}
