// feature_extraction.cpp -- so_icp_extract_features(_dev): featureExtraction's per-sweep path (laserCloudHandler's ingest,
// removePointDistortion, uniformFeatureExtraction; src/FeatureExtraction/featureExtraction.cpp) as one enqueue on the device.
//
// The node's bookkeeping around it (frame skipping, the sweep and pose buffers, the branch choice, the LaserFeature message) stays
// with the caller; this entry takes one sweep and the pose buffer the branch chose, and returns cloud_nodistortion and
// cloud_surface.  Kernels: feature_kernels.hip.  The per-scan de-skew constants are deskew_setup's, as for so_icp_deskew_scan.
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "deskew_math.h"
#include "feature_kernels.h"

namespace {

// device state of the entry, owned by the context (so_icp_ctx::fe_state)
struct FeatureState {
  DevBuf raw;     // the payload (host entry)
  DevBuf rec;     // cloud_nodistortion
  DevBuf surf;    // cloud_surface
  DevBuf small;   // counters {n_clamped, n_surface, ticket, -} | look-back words of the compaction | pose table
  uint32_t* h_counts = nullptr;  // pinned read-back of {n_clamped, n_surface}
  ~FeatureState() {
    for (DevBuf* b : {&raw, &rec, &surf, &small}) b->release();
    if (h_counts) (void)hipHostFree(h_counts);
  }
};

int check_layout(so_icp_ctx* c, const char* who, uint32_t width, uint32_t height, const so_icp_sweep_layout* L) {
  const std::string w(who);
  if (L->sensor != SO_ICP_SENSOR_VELODYNE && L->sensor != SO_ICP_SENSOR_OUSTER)
    return fail(c, SO_ICP_E_INVALID, w + ": unknown sensor (SO_ICP_SENSOR_VELODYNE or SO_ICP_SENSOR_OUSTER)");
  if (L->is_bigendian) return fail(c, SO_ICP_E_INVALID, w + ": big-endian payloads are not supported");
  if (L->filter_point_size < 1) return fail(c, SO_ICP_E_INVALID, w + ": filter_point_size must be >= 1");
  if (L->point_step == 0) return fail(c, SO_ICP_E_INVALID, w + ": point_step must be > 0");
  if ((uint64_t)L->row_step < (uint64_t)width * L->point_step) return fail(c, SO_ICP_E_INVALID, w + ": row_step < width * point_step");
  const bool ouster = L->sensor == SO_ICP_SENSOR_OUSTER;
  const struct { int32_t off; uint32_t bytes; const char* name; } f[] = {
      {L->off_x, 4, "x"}, {L->off_y, 4, "y"}, {L->off_z, 4, "z"}, {L->off_intensity, 4, "intensity"}, {L->off_time, 4, "time"},
      {ouster ? -1 : L->off_ring, 2, "ring"}};
  for (const auto& q : f)
    if (q.off < -1 || (q.off >= 0 && (uint64_t)q.off + q.bytes > L->point_step))
      return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " lies past point_step");
  if ((uint64_t)width * height >= ((uint64_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, w + ": too many points");
  return SO_ICP_OK;
}

SweepFields fields_of(const so_icp_sweep_layout* L, uint32_t width) {
  SweepFields sf;
  sf.point_step = L->point_step; sf.row_step = L->row_step; sf.width = width;
  sf.x = L->off_x; sf.y = L->off_y; sf.z = L->off_z; sf.intensity = L->off_intensity; sf.time = L->off_time;
  sf.ouster = L->sensor == SO_ICP_SENSOR_OUSTER ? 1 : 0;
  sf.ring = sf.ouster ? -1 : L->off_ring;
  for (int k = 0; k < 3; ++k) sf.ouster_t[k] = L->T_ouster_sensor[k];
  for (int k = 0; k < 4; ++k) sf.ouster_q[k] = L->T_ouster_sensor[3 + k];
  return sf;
}

int check_args(so_icp_ctx* c, const char* who, const void* raw, uint32_t width, uint32_t height, const so_icp_sweep_layout* L,
               const so_icp_stamped_pose* poses, size_t n_poses) {
  if (!c || !L || (!raw && (uint64_t)width * height) || (n_poses && !poses)) return SO_ICP_E_INVALID;
  if (const int rc = check_layout(c, who, width, height, L)) return rc;
  if (n_poses >= ((size_t)1 << 24)) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(who) + ": too many poses");
  NEED_DEVICE(c);
  return SO_ICP_OK;
}

// the whole pass on queue s: [payload copy], counters cleared, pose table, ingest + de-skew, compaction, counts read back
int run(so_icp_ctx* c, hipStream_t s, FeatureState& st, const uint8_t* d_raw, uint32_t n, const so_icp_sweep_layout* L, uint32_t width,
        double t0, const so_icp_stamped_pose* poses, size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info) {
  static_assert(sizeof(so_icp_stamped_pose) == kStampedPoseDoubles * sizeof(double), "stamped pose = 8 doubles");
  std::memset(&info, 0, sizeof(info));
  info.q_w_original_l[3] = 1.0;
  info.n_points = n;
  DeskewFrames f{};
  std::vector<double> tab;
  if (n_poses) {
    if (!deskew_setup(reinterpret_cast<const double*>(poses), n_poses, t0, imu, T_i_l, f, tab, info.q_w_original_l, info.t_w_original_l))
      return fail(c, SO_ICP_E_INVALID, "pose buffer times must increase strictly (the reference keeps them in a std::map)");
    info.deskewed = 1;
  }
  if (!n) return SO_ICP_OK;
  const uint32_t step = (uint32_t)L->filter_point_size, nblk = surf_workgroups(n, step);
  const size_t state_off = 16, tab_off = (state_off + (size_t)nblk * 8 + 255) & ~(size_t)255;
  HIP_TRY(c, st.rec.reserve((size_t)n * kFeatureRecordBytes));
  HIP_TRY(c, st.surf.reserve((size_t)(surf_candidates(n, step) + 1) * kFeatureRecordBytes));
  HIP_TRY(c, st.small.reserve(tab_off + tab.size() * sizeof(double) + 64));
  if (!st.h_counts) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&st.h_counts), 64));
  uint32_t* d_counts = st.small.as<uint32_t>();
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, tab_off, s));
  if (n_poses) HIP_TRY(c, hipMemcpyAsync(st.small.as<uint8_t>() + tab_off, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  launch_ingest_deskew(d_raw, n, fields_of(L, width), st.rec.as<uint8_t>(), t0, reinterpret_cast<const double*>(st.small.as<uint8_t>() + tab_off),
                       (uint32_t)n_poses, f, d_counts, s);
  launch_surf_sample(st.rec.as<uint8_t>(), n, step, L->min_range, st.surf.as<uint8_t>(), d_counts + 1,
                     reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), d_counts + 2, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_counts, d_counts, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // (also keeps `tab` alive until its upload has been consumed)
  info.n_clamped = st.h_counts[0];
  info.n_surface = st.h_counts[1];
  return SO_ICP_OK;
}

FeatureState* state_of(so_icp_ctx* c) {
  if (!c->fe_state) c->fe_state = std::make_shared<FeatureState>();
  return static_cast<FeatureState*>(c->fe_state.get());
}

}  // namespace

extern "C" {

int so_icp_extract_features(so_icp_ctx* c, const void* raw, uint32_t width, uint32_t height, const so_icp_sweep_layout* L, double lidar_start_time,
                            const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7], void* nodistortion_out,
                            void* surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features", raw, width, height, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));  // (before the auxiliary queue may be created: on the context's device)
  FeatureState& st = *state_of(c);
  hipStream_t s = aux_stream(c);  // (a host buffer in, host buffers out: the queue of the other steps around Localization())
  const uint32_t n = width * height;
  if (n) {
    const size_t bytes = (size_t)L->row_step * (height - 1) + (size_t)width * L->point_step;  // (the last row's tail is never read)
    HIP_TRY(c, st.raw.reserve(bytes + 64));
    // straight from the caller's buffer, as so_icp_prefilter_scan copies its cloud: a copy into a pinned staging buffer first
    // made the call slower (0.419 against 0.289 ms for the 131 072-point Ouster sweep) -- the runtime already
    // pipelines a pageable copy through its own pinned chunks
    HIP_TRY(c, hipMemcpyAsync(st.raw.p, raw, bytes, hipMemcpyHostToDevice, s));
  }
  so_icp_feature_info li;
  const int rc = run(c, s, st, st.raw.as<uint8_t>(), n, L, width, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, li);
  if (rc) return rc;
  if (n && nodistortion_out) HIP_TRY(c, hipMemcpyAsync(nodistortion_out, st.rec.p, (size_t)n * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  if (li.n_surface && surface_out) HIP_TRY(c, hipMemcpyAsync(surface_out, st.surf.p, (size_t)li.n_surface * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (info) *info = li;
  return SO_ICP_OK;
}

int so_icp_extract_features_dev(so_icp_ctx* c, const void* d_raw, uint32_t width, uint32_t height, const so_icp_sweep_layout* L,
                                double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7],
                                void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features_dev", d_raw, width, height, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  so_icp_feature_info li;
  // (the caller's device buffer: the context's queue, as so_icp_deskew_scan_dev)
  const int rc = run(c, c->stream, st, static_cast<const uint8_t*>(d_raw), width * height, L, width, lidar_start_time, poses, n_poses,
                     poses_are_imu, T_i_l, li);
  if (rc) return rc;
  if (d_nodistortion_out) *d_nodistortion_out = st.rec.p;
  if (d_surface_out) *d_surface_out = st.surf.p;
  if (info) *info = li;
  return SO_ICP_OK;
}

}  // extern "C"
