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
// --correspondences: the frames as without a flag, with LidarSLAM::keep_correspondences on; behind the output above, the last frame's
//          correspondence set (LidarSLAM::LastCorrespondences at the optimised pose): the so_icp_correspondence_info as it is, then
//          n_accepted so_icp_correspondence records as they are
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
    slam.keep_correspondences = correspondences;
    bool initialization = false;                        // laserMapping.cpp: first frame seeds the map
    for (int f = 0; f < n_frames; ++f) {
      if (f + 1 < n_frames && f >= 1) slam.StageNextScan(clouds[f + 1]);  // what the feature callback would do
      slam.Localization(initialization, LidarSLAM::PredictionSource::LIO_ODOM, guesses[f], edge, clouds[f], times[f]);
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
