// localization.cpp -- so_icp_localization(_dev): one frame of LidarSLAM::Localization (seed the map, or registration,
// checkMotionThresholds and the map insert) from a scan in host memory or one resident in HBM.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "ctx.h"

namespace {

// Where the frame's scan is: a host buffer with its stride (so_icp_localization) or packed xyz in HBM (so_icp_localization_dev)
struct FrameScan {
  bool on_host;
  const float* xyz;     // host: the caller's buffer; resident: the device address
  size_t n, stride_bytes;
};

// The intensities that go with a frame's scan (so_icp_set_cloud_intensity): in the caller's host records, or a device array of n floats
// (the last pre-filter's, when the resident scan is its output), or none -- the map then takes 0
struct FrameIntensity { const float* host = nullptr; size_t stride_floats = 0; const float* dev = nullptr; };

FrameIntensity frame_intensity(const so_icp_ctx* c, const FrameScan& s) {
  FrameIntensity fi;
  if (c->intensity_off < 0) return fi;
  if (s.on_host) { fi.host = intensity_in(c, s.xyz, s.stride_bytes); fi.stride_floats = s.stride_bytes / 4; }
  else if (c->pf_inten_on && s.xyz == c->pf_out.as<float>() && s.n == c->pf_inten_n) fi.dev = c->pf_inten.as<float>();
  return fi;
}

// transformAndAddToMap (LidarSlam.cpp:60-80) entirely on the device: one launch transforms the scan, finds every point's cube and
// lays the insert round out; the insert is enqueued without a read-back and -- unless SOICP_MAP_FAST=sync -- completes behind
// this call (device_map.h, settle)
int insert_resident(so_icp_ctx* c, const float* d_scan, size_t n, const double T[7], const FrameIntensity& fi) {
  if (const int rs = map_status(c->dmap->settle(c->err))) return rs;  // (before d_world may be re-allocated)
  HIP_TRY(c, c->d_world.reserve((n + 64) * 16));  // world x y z, and behind them the intensities (transformAndAddToMap copies the point and rewrites x y z)
  const float* d_inten = fi.dev;
  if (fi.host && n) {
    // gathered from the caller's records into pinned memory and sent down the context's queue in front of the insert (the insert
    // before this one has been settled: nothing reads either buffer any more)
    if (c->h_inten_cap < n) {
      if (c->h_inten) (void)hipHostFree(c->h_inten);
      c->h_inten = nullptr; c->h_inten_cap = 0;
      HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_inten), (n + n / 4 + 64) * sizeof(float)));
      c->h_inten_cap = n + n / 4 + 64;
    }
    for (size_t i = 0; i < n; ++i) c->h_inten[i] = fi.host[i * fi.stride_floats];
    HIP_TRY(c, c->d_inten.reserve(n * sizeof(float) + 64));
    HIP_TRY(c, hipMemcpyAsync(c->d_inten.p, c->h_inten, n * sizeof(float), hipMemcpyHostToDevice, c->stream));
    d_inten = c->d_inten.as<float>();
  }
  const int r = c->dmap->add_scan_dev(d_scan, n, T, c->d_world.as<float>(), c->dmap->defer_enabled() && !c->dmap->sharded(), c->err, d_inten,
                                      c->d_world.as<float>() + 3 * (n + 64));
  return r < 0 ? map_status(r) : exchange_map_counts(c);
}

// transformAndAddToMap with the transform on the host, in double (TransformPoint, superodom_utils.h:119-123)
int insert_from_host(so_icp_ctx* c, const float* xyz, size_t n, size_t sf, const double T[7], const FrameIntensity& fi) {
  std::vector<float> w(n * 3);
  for (size_t i = 0; i < n; ++i) {
    double ox, oy, oz;
    quat_rotate<double>(T + 3, (double)xyz[i * sf], (double)xyz[i * sf + 1], (double)xyz[i * sf + 2], ox, oy, oz);
    w[3 * i] = (float)(ox + T[0]); w[3 * i + 1] = (float)(oy + T[1]); w[3 * i + 2] = (float)(oz + T[2]);
  }
  if (c->dmap) { const int r = c->dmap->add_surf_host(w.data(), n, 3, c->err, fi.host, fi.stride_floats); return r < 0 ? map_status(r) : exchange_map_counts(c); }
  return c->map.add_surf(w.data(), n, 3) < 0 ? fail(c, SO_ICP_E_INVALID, "LocalMap insert failed") : SO_ICP_OK;
}

// checkMotionThresholds, LidarSlam.cpp:173-195: always accepts; only the startupCount side effect survives
void accept_frame(so_icp_ctx* c, so_icp_stats* st, double time) {
  const double dt = time - c->last_time;
  if (st->translation_from_last / dt > c->cfg.velocity_failure_threshold) c->startup_count = 5;
  st->startup_count = c->startup_count;
}

// Registration, checkMotionThresholds and the insert of the scan at d_scan (LidarSlam.cpp:96-170)
int register_and_insert(so_icp_ctx* c, const FrameScan& s, const float* d_scan, const double T_in[7], double time, double pose_out[7],
                        so_icp_stats* st) {
  int rc = register_core(c, d_scan, s.n, T_in, pose_out, st);
  if (s.on_host) c->scan_staged = false;  // (set by resolve_scan for this registration only)
  if (rc != SO_ICP_OK) return rc;  // NOT_ENOUGH: the reference returns before the post-processing (LidarSlam.cpp:113-116)
  accept_frame(c, st, time);
  // The insert, LidarSlam.cpp:163-167.  With a device map it reads the copy the registration ran on, which is still resident -- the
  // caller's, a stage slot or d_scan_own --, never the host buffer; without one the points are needed on the host (the resident entry
  // has handed such a context to the host entry)
  const FrameIntensity fi = frame_intensity(c, s);
  rc = c->dmap ? insert_resident(c, d_scan, s.n, pose_out, fi) : insert_from_host(c, s.xyz, s.n, s.stride_bytes / 4, pose_out, fi);
  if (rc) return rc;
  c->last_time = time;
  return SO_ICP_OK;
}

// One frame of Localization(): seed the map (initializeMapping), or register + accept + insert
int localization_frame(so_icp_ctx* c, int initialization, const double T_in[7], const FrameScan& s, double time, double pose_out[7],
                       so_icp_stats* st) {
  c->corr_last.valid = false;  // (so_icp_correspondences: set again by a registration that ends with SO_ICP_OK)
  if (!initialization) {  // initializeMapping, LidarSlam.cpp:83-94
    std::memcpy(pose_out, T_in, 7 * sizeof(double));
    if (st) std::memset(st, 0, sizeof(*st));
    // The host entry seeds from the host buffer, transformed on the host -- on a host-only context too, and also where a device map
    // exists --, and a staged copy of that buffer is dropped; the resident entry seeds on the device.  (Nothing shows that the two
    // transforms give the same bits: neither is routed through the other.)
    if (s.on_host && !c->host_only) drop_staged(c, s.xyz, s.n, s.stride_bytes);
    if (c->dmap) c->dmap->set_origin(T_in); else c->map.set_origin(T_in);
    const FrameIntensity fi = frame_intensity(c, s);
    const int r = s.on_host ? insert_from_host(c, s.xyz, s.n, s.stride_bytes / 4, T_in, fi) : insert_resident(c, s.xyz, s.n, T_in, fi);
    if (r) return r;
    c->last_time = time;
    return SO_ICP_MAP_SEEDED;
  }
  so_icp_stats local;
  if (!st) st = &local;
  NEED_DEVICE(c);
  if (!s.on_host) return register_and_insert(c, s, s.xyz, T_in, time, pose_out, st);
  // A host scan: its staged copy, or an upload into d_scan_own; the stage slot is released on every way out after resolve_scan
  const float* d_scan = nullptr;
  if (const int rc = resolve_scan(c, s.xyz, s.n, s.stride_bytes, &d_scan)) return rc;
  const int rc = register_and_insert(c, s, d_scan, T_in, time, pose_out, st);
  release_staged(c);
  return rc;
}

}  // namespace

extern "C" {

int so_icp_localization(so_icp_ctx* c, int initialization, const double T_in[7], const float* xyz, size_t n, size_t stride_bytes,
                        double time_laser_odometry, double pose_out[7], so_icp_stats* st) {
  if (!c) return SO_ICP_E_INVALID;
  if (const int rc = refuse_pending(c, "so_icp_localization", kPriorSingle)) return rc;
  const PriorOneShot consume{c};  // (a frame that seeds the map consumes it too)
  if (!T_in || !pose_out || (!xyz && n)) return SO_ICP_E_INVALID;
  if (const int rc = normalise_stride(c, &stride_bytes)) return rc;
  if (!c->host_only) HIP_TRY(c, hipSetDevice(c->cfg.device_id));  // (the caller may sit on another device / thread)
  return localization_frame(c, initialization, T_in, FrameScan{true, xyz, n, stride_bytes}, time_laser_odometry, pose_out, st);
}

int so_icp_localization_dev(so_icp_ctx* c, int initialization, const double T_in[7], const void* d_scan, size_t n,
                            double time_laser_odometry, double pose_out[7], so_icp_stats* st) {
  if (!c) return SO_ICP_E_INVALID;
  if (const int rc = refuse_pending(c, "so_icp_localization_dev", kPriorSingle)) return rc;
  const PriorOneShot consume{c};
  if (!T_in || !pose_out || (!d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (!c->dmap) {  // host-side LocalMap (sharded ranks): the insert needs the points on the host
    std::vector<float> h(n * 3);
    const int rc = so_icp_download_scan(c, d_scan, n, h.data());
    if (rc) return rc;
    return so_icp_localization(c, initialization, T_in, h.data(), n, 12, time_laser_odometry, pose_out, st);
  }
  return localization_frame(c, initialization, T_in, FrameScan{false, static_cast<const float*>(d_scan), n, 12}, time_laser_odometry, pose_out, st);
}

}  // extern "C"
