// feature_driver.cpp -- runs the feature_extraction_node shell (feature_extraction_soicp.{h,cpp}) over a recorded stream of
// serialised sensor_msgs/PointCloud2 sweeps and pose measurements, the way a rosbag2 replay feeds the reference node, and
// records the LaserFeature messages it publishes (test binary: built by __graft_entry__.build(), run by
// tests/test_gpu_feature_node.py; the configuration check runs without a GPU in tests/test_feature_extraction_host.py).
//
//   feature_driver <params.yaml> <bag.bin> <out.bin>
// bag.bin: int32 IMU_INIT, 7 doubles T_i_l (tx ty tz qx qy qz qw), int32 n_events; per event: uint8 kind and
//          kind 0: uint32 length + CDR bytes of a PointCloud2 (laserCloudHandler)
//          kind 1: double t, double q[4] x y z w (an IMU orientation)
//          kind 2: double t, double pos[3], double q[4] (a VIO pose)
// out.bin: per published message: uint32 event, uint32 len + topic, uint32 len + type, uint32 len + CDR bytes;
//          trailer: uint32 0xFFFFFFFF, int32 frames_failed, uint32 len + last error text
#include <cstdint>
#include <cstdio>
#include <stdexcept>

#include "feature_extraction_soicp.h"

using namespace super_odometry_soicp;

template <typename T> static T rd(FILE* f) { T v; if (fread(&v, sizeof(T), 1, f) != 1) throw std::runtime_error("short input"); return v; }
template <typename T> static void wr(FILE* f, const T& v) { fwrite(&v, sizeof(T), 1, f); }
static void wr_blob(FILE* f, const void* p, size_t n) { wr<uint32_t>(f, (uint32_t)n); fwrite(p, 1, n, f); }

struct Recorder : Outbox {
  FILE* f = nullptr;
  uint32_t event = 0;
  void publish(const std::string& topic, const std::string& type, std::vector<uint8_t>&& cdr) override {
    wr<uint32_t>(f, event); wr_blob(f, topic.data(), topic.size()); wr_blob(f, type.data(), type.size()); wr_blob(f, cdr.data(), cdr.size());
  }
};

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: %s params.yaml bag.bin out.bin\n", argv[0]); return 2; }
  try {
    FeatureConfig cfg = load_feature_config(argv[1]);
    FILE* in = fopen(argv[2], "rb");
    if (!in) throw std::runtime_error("cannot open the bag");
    const int32_t imu_init = rd<int32_t>(in);
    for (double& v : cfg.T_i_l) v = rd<double>(in);
    Recorder rec;
    featureExtraction node(cfg, &rec);  // (refuses what the shell does not restate before the output file is created)
    rec.f = fopen(argv[3], "wb");
    if (!rec.f) throw std::runtime_error("cannot open the output");
    node.IMU_INIT = imu_init != 0;
    const int32_t n_events = rd<int32_t>(in);
    for (int32_t k = 0; k < n_events; ++k) {
      rec.event = (uint32_t)k;
      const uint8_t kind = rd<uint8_t>(in);
      if (kind == 0) {
        std::vector<uint8_t> b(rd<uint32_t>(in));
        if (!b.empty() && fread(b.data(), 1, b.size(), in) != b.size()) throw std::runtime_error("short message");
        node.laserCloudHandler(so_wire::deserialize<so_wire::PointCloud2>(b));
      } else if (kind == 1) {
        const double t = rd<double>(in);
        double q[4];
        for (double& v : q) v = rd<double>(in);
        node.addImuOrientation(t, q);
      } else if (kind == 2) {
        const double t = rd<double>(in);
        double p[3], q[4];
        for (double& v : p) v = rd<double>(in);
        for (double& v : q) v = rd<double>(in);
        node.addVisualOdometry(t, p, q);
      } else {
        throw std::runtime_error("unknown event kind");
      }
    }
    wr<uint32_t>(rec.f, 0xFFFFFFFFu); wr<int32_t>(rec.f, node.frames_failed); wr_blob(rec.f, node.last_error.data(), node.last_error.size());
    fclose(in); fclose(rec.f);
  } catch (const std::exception& e) {
    fprintf(stderr, "feature_driver: %s\n", e.what());
    return 1;
  }
  return 0;
}
