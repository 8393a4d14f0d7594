// feature_extraction.cpp -- so_icp_extract_features(_dev), so_icp_extract_features_livox(_dev) and so_icp_extract_features_untimed(_dev):
// featureExtraction's per-sweep path (laserCloudHandler's, livoxHandler's or assignTimeforPointCloud's ingest, removePointDistortion, uniformFeatureExtraction;
// src/FeatureExtraction/featureExtraction.cpp) as one enqueue on the device.
//
// The node's bookkeeping around it (frame skipping, the sweep and pose buffers, the branch choice, the LaserFeature message) stays
// with the caller; this entry takes one sweep and the pose buffer the branch chose, and returns cloud_nodistortion and
// cloud_surface.  Kernels: feature_kernels.hip.  The per-scan de-skew constants are deskew_setup's, as for so_icp_deskew_scan.
//
// so_icp_registered_scan(_dev) closes the resident chain behind them: laserMapping::publishTopic's registered scan
// (src/LaserMapping/laserMapping.cpp:464-493) from the records that pass left in HBM, transformed and compacted in one launch.
#include <algorithm>
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

// the fields of a CustomPoint in so_icp_livox_layout: offset, bytes, name
struct LivoxField { int32_t off; uint32_t bytes; const char* name; };
inline void livox_fields(const so_icp_livox_layout* L, LivoxField f[7]) {
  const LivoxField v[7] = {{L->off_offset_time, 4, "offset_time"}, {L->off_x, 4, "x"}, {L->off_y, 4, "y"}, {L->off_z, 4, "z"},
                           {L->off_reflectivity, 1, "reflectivity"}, {L->off_tag, 1, "tag"}, {L->off_line, 1, "line"}};
  for (int k = 0; k < 7; ++k) f[k] = v[k];
}

int check_livox_layout(so_icp_ctx* c, const char* who, uint32_t n, const so_icp_livox_layout* L) {
  const std::string w(who);
  if (L->filter_point_size < 1) return fail(c, SO_ICP_E_INVALID, w + ": filter_point_size must be >= 1");
  if (L->n_scans < 0 || L->n_scans > 256) return fail(c, SO_ICP_E_INVALID, w + ": n_scans must lie in 0 .. 256 (line is a uint8)");
  if (L->point_step == 0) return fail(c, SO_ICP_E_INVALID, w + ": point_step must be > 0");
  LivoxField f[7];
  livox_fields(L, f);
  for (const LivoxField& q : f) {
    if (q.off < 0) return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " must be >= 0 (a CustomPoint has every field)");
    if ((uint64_t)q.off + q.bytes > L->point_step) return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " lies past point_step");
  }
  if (n >= ((uint32_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, w + ": too many points");
  return SO_ICP_OK;
}

LivoxFields livox_fields_of(const so_icp_livox_layout* L) {
  LivoxFields lf;
  lf.point_step = L->point_step;
  lf.offset_time = (uint32_t)L->off_offset_time; lf.x = (uint32_t)L->off_x; lf.y = (uint32_t)L->off_y; lf.z = (uint32_t)L->off_z;
  lf.reflectivity = (uint32_t)L->off_reflectivity; lf.tag = (uint32_t)L->off_tag; lf.line = (uint32_t)L->off_line;
  lf.n_scans = (uint32_t)L->n_scans;
  for (int k = 0; k < 9; ++k) lf.R[k] = L->R_imu_laser_gravity[k];
  return lf;
}

// bytes of the payload that are read: the last point ends with its last field (19 of the 20 bytes of a CDR CustomPoint)
size_t livox_payload_bytes(uint32_t n, const so_icp_livox_layout* L) {
  LivoxField f[7];
  livox_fields(L, f);
  size_t end = 0;
  for (const LivoxField& q : f) end = std::max(end, (size_t)q.off + q.bytes);
  return n ? (size_t)(n - 1) * L->point_step + end : 0;
}

int check_livox_args(so_icp_ctx* c, const char* who, const void* raw, uint32_t n, const so_icp_livox_layout* L, const so_icp_stamped_pose* poses,
                     size_t n_poses) {
  if (!c || !L || (!raw && n) || (n_poses && !poses)) return SO_ICP_E_INVALID;
  if (const int rc = check_livox_layout(c, who, n, L)) return rc;
  if (n_poses >= ((size_t)1 << 24)) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(who) + ": too many poses");
  NEED_DEVICE(c);
  return SO_ICP_OK;
}

// the whole pass on queue s: [payload copy], counters cleared, pose table, ingest + de-skew, compaction, counts read back.
// ingest(d_rec, d_pose_table, frames, d_n_clamped): the sensor's launch_*ingest_deskew on queue s; step, min_range: the sampler's.
template <typename Ingest>
int run(so_icp_ctx* c, hipStream_t s, FeatureState& st, uint32_t n, uint32_t step, float min_range, double t0, const so_icp_stamped_pose* poses,
        size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info, Ingest&& ingest) {
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
  const uint32_t nblk = surf_workgroups(n, step);
  const size_t state_off = 16, tab_off = (state_off + (size_t)nblk * 8 + 255) & ~(size_t)255;
  HIP_TRY(c, st.rec.reserve((size_t)n * kFeatureRecordBytes));
  HIP_TRY(c, st.surf.reserve((size_t)(surf_candidates(n, step) + 1) * kFeatureRecordBytes));
  HIP_TRY(c, st.small.reserve(tab_off + tab.size() * sizeof(double) + 64));
  if (!st.h_counts) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&st.h_counts), 64));
  uint32_t* d_counts = st.small.as<uint32_t>();
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, tab_off, s));
  if (n_poses) HIP_TRY(c, hipMemcpyAsync(st.small.as<uint8_t>() + tab_off, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  ingest(st.rec.as<uint8_t>(), reinterpret_cast<const double*>(st.small.as<uint8_t>() + tab_off), f, d_counts);
  launch_surf_sample(st.rec.as<uint8_t>(), n, step, min_range, st.surf.as<uint8_t>(), d_counts + 1,
                     reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), d_counts + 2, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_counts, d_counts, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // (also keeps `tab` alive until its upload has been consumed)
  info.n_clamped = st.h_counts[0];
  info.n_surface = st.h_counts[1];
  return SO_ICP_OK;
}

// run() for a PointCloud2 sweep (laserCloudHandler) and for a CustomMsg's points (livoxHandler)
int run_sweep(so_icp_ctx* c, hipStream_t s, FeatureState& st, const uint8_t* d_raw, uint32_t n, const so_icp_sweep_layout* L, uint32_t width,
              double t0, const so_icp_stamped_pose* poses, size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info) {
  return run(c, s, st, n, (uint32_t)L->filter_point_size, L->min_range, t0, poses, n_poses, imu, T_i_l, info,
             [&](uint8_t* d_rec, const double* d_tab, const DeskewFrames& f, uint32_t* d_n_clamped) {
               launch_ingest_deskew(d_raw, n, fields_of(L, width), d_rec, t0, d_tab, (uint32_t)n_poses, f, d_n_clamped, s);
             });
}
int run_livox(so_icp_ctx* c, hipStream_t s, FeatureState& st, const uint8_t* d_raw, uint32_t n, const so_icp_livox_layout* L, double t0,
              const so_icp_stamped_pose* poses, size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info) {
  return run(c, s, st, n, (uint32_t)L->filter_point_size, L->min_range, t0, poses, n_poses, imu, T_i_l, info,
             [&](uint8_t* d_rec, const double* d_tab, const DeskewFrames& f, uint32_t* d_n_clamped) {
               launch_livox_ingest_deskew(d_raw, n, livox_fields_of(L), d_rec, t0, d_tab, (uint32_t)n_poses, f, d_n_clamped, s);
             });
}

// ---- so_icp_extract_features_untimed(_dev): a sweep without per-point time (assignTimeforPointCloud, :646-708) ----
int check_untimed_layout(so_icp_ctx* c, const char* who, uint32_t width, uint32_t height, const so_icp_untimed_layout* L) {
  const std::string w(who);
  if (L->is_bigendian) return fail(c, SO_ICP_E_INVALID, w + ": big-endian payloads are not supported");
  if (L->filter_point_size < 1) return fail(c, SO_ICP_E_INVALID, w + ": filter_point_size must be >= 1");
  bool scans_ok = false;
  for (int32_t v : {4, 16, 32, 64, 128}) scans_ok = scans_ok || L->n_scans == v;  // featureExtraction.cpp:62
  if (!scans_ok) return fail(c, SO_ICP_E_INVALID, w + ": n_scans must be 4, 16, 32, 64 or 128");
  if (L->point_step == 0) return fail(c, SO_ICP_E_INVALID, w + ": point_step must be > 0");
  if ((uint64_t)L->row_step < (uint64_t)width * L->point_step) return fail(c, SO_ICP_E_INVALID, w + ": row_step < width * point_step");
  const struct { int32_t off; const char* name; } f[] = {{L->off_x, "x"}, {L->off_y, "y"}, {L->off_z, "z"}, {L->off_intensity, "intensity"}};
  for (const auto& q : f)
    if (q.off < -1 || (q.off >= 0 && (uint64_t)q.off + 4 > L->point_step))
      return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " lies past point_step");
  if ((uint64_t)width * height >= ((uint64_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, w + ": too many points");
  return SO_ICP_OK;
}

int check_untimed_args(so_icp_ctx* c, const char* who, const void* raw, uint32_t width, uint32_t height, const so_icp_untimed_layout* L,
                       const so_icp_stamped_pose* poses, size_t n_poses) {
  if (!c || !L || (!raw && (uint64_t)width * height) || (n_poses && !poses)) return SO_ICP_E_INVALID;
  if (const int rc = check_untimed_layout(c, who, width, height, L)) return rc;
  if (n_poses >= ((size_t)1 << 24)) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(who) + ": too many poses");
  NEED_DEVICE(c);
  return SO_ICP_OK;
}

UntimedFields untimed_fields_of(const so_icp_untimed_layout* L, uint32_t width) {
  UntimedFields uf;
  uf.point_step = L->point_step; uf.row_step = L->row_step; uf.width = width;
  uf.x = L->off_x; uf.y = L->off_y; uf.z = L->off_z; uf.intensity = L->off_intensity;
  uf.n_scans = (uint32_t)L->n_scans;
  return uf;
}

// run() for such a sweep.  The number of records is known only on the device and surf_sample_kernel takes it as a launch
// argument, so it is read back between the two launches: counters cleared, pose table, ingest + compaction + de-skew, the counts
// read back (wait), the sampler over the n_kept records, its count read back (wait).
int run_untimed(so_icp_ctx* c, hipStream_t s, FeatureState& st, const uint8_t* d_raw, uint32_t n, const so_icp_untimed_layout* L, uint32_t width,
                double t0, const so_icp_stamped_pose* poses, size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info) {
  std::memset(&info, 0, sizeof(info));  // what stays where there is no record: zero counts, no de-skew, the identity
  info.q_w_original_l[3] = 1.0;
  DeskewFrames f{};
  std::vector<double> tab;
  double q_start[4] = {0.0, 0.0, 0.0, 1.0}, t_start[3] = {0.0, 0.0, 0.0};  // the sweep-start pose, reported once a record exists
  if (n_poses && !deskew_setup(reinterpret_cast<const double*>(poses), n_poses, t0, imu, T_i_l, f, tab, q_start, t_start))
    return fail(c, SO_ICP_E_INVALID, "pose buffer times must increase strictly (the reference keeps them in a std::map)");
  if (!n) return SO_ICP_OK;
  const uint32_t step = (uint32_t)L->filter_point_size;
  // counters {n_clamped, n_surface, sampler's ticket, -, n_kept, ingest's ticket, -, -} | the sampler's look-back words (for up to
  // n records) | the ingest's | pose table
  const size_t surf_state_off = 32, in_state_off = surf_state_off + (size_t)surf_workgroups(n, step) * 8,
               tab_off = (in_state_off + (size_t)untimed_workgroups(n) * 8 + 255) & ~(size_t)255;
  HIP_TRY(c, st.rec.reserve((size_t)n * kFeatureRecordBytes));
  HIP_TRY(c, st.surf.reserve((size_t)(surf_candidates(n, step) + 1) * kFeatureRecordBytes));
  HIP_TRY(c, st.small.reserve(tab_off + tab.size() * sizeof(double) + 64));
  if (!st.h_counts) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&st.h_counts), 64));
  uint32_t* d_counts = st.small.as<uint32_t>();
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, tab_off, s));
  if (n_poses) HIP_TRY(c, hipMemcpyAsync(st.small.as<uint8_t>() + tab_off, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  launch_untimed_ingest_deskew(d_raw, n, untimed_fields_of(L, width), st.rec.as<uint8_t>(), t0,
                               reinterpret_cast<const double*>(st.small.as<uint8_t>() + tab_off), (uint32_t)n_poses, f, d_counts, d_counts + 4,
                               reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + in_state_off), d_counts + 5, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_counts, d_counts, 32, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // (also keeps `tab` alive until its upload has been consumed)
  const uint32_t n_kept = st.h_counts[4];
  if (!n_kept) return SO_ICP_OK;
  info.n_points = n_kept;
  info.n_clamped = st.h_counts[0];
  if (n_poses) {
    info.deskewed = 1;
    std::memcpy(info.q_w_original_l, q_start, sizeof(q_start));
    std::memcpy(info.t_w_original_l, t_start, sizeof(t_start));
  }
  if (!surf_workgroups(n_kept, step)) return SO_ICP_OK;  // one record: no candidate
  launch_surf_sample(st.rec.as<uint8_t>(), n_kept, step, L->min_range, st.surf.as<uint8_t>(), d_counts + 1,
                     reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + surf_state_off), d_counts + 2, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_counts + 1, d_counts + 1, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  info.n_surface = st.h_counts[1];
  return SO_ICP_OK;
}

// the clouds of the host entries: out of the context's buffers into the caller's
int read_back(so_icp_ctx* c, hipStream_t s, FeatureState& st, const so_icp_feature_info& li, void* nodistortion_out, void* surface_out) {
  if (li.n_points && nodistortion_out) HIP_TRY(c, hipMemcpyAsync(nodistortion_out, st.rec.p, (size_t)li.n_points * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  if (li.n_surface && surface_out) HIP_TRY(c, hipMemcpyAsync(surface_out, st.surf.p, (size_t)li.n_surface * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SO_ICP_OK;
}

// device state of so_icp_registered_scan(_dev), owned by the context (so_icp_ctx::rs_state): nothing of it is the feature
// extraction's or the pre-filter's, so those entries leave *d_out alone and this one leaves their clouds alone
struct RegisteredScanState {
  DevBuf in;     // the records (host entry)
  DevBuf out;    // the registered scan
  DevBuf small;  // counters {n_kept, ticket, -, -} | look-back words of the compaction
  uint32_t* h_kept = nullptr;  // pinned read-back of n_kept
  ~RegisteredScanState() {
    for (DevBuf* b : {&in, &out, &small}) b->release();
    if (h_kept) (void)hipHostFree(h_kept);
  }
};

int check_registered_scan_args(so_icp_ctx* c, const void* records, size_t n, size_t stride, const double T[7], bool on_device) {
  if (!c || !T || (!records && n)) return SO_ICP_E_INVALID;
  if (stride < 12 || stride % 4) return fail(c, SO_ICP_E_INVALID, "records: float x y z at 0 4 8, stride a multiple of 4");
  if (on_device && reinterpret_cast<uintptr_t>(records) % 4u) return fail(c, SO_ICP_E_INVALID, "records: the device address must be 4-byte aligned");
  if (n >= ((size_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, "too many points");
  NEED_DEVICE(c);
  return SO_ICP_OK;
}

// on queue s: counters and look-back words cleared, one launch, [the copy to `out`] and the count enqueued together, one wait
int run_registered_scan(so_icp_ctx* c, hipStream_t s, RegisteredScanState& st, const uint8_t* d_rec, size_t n, size_t stride, const double T[7],
                        void* out, size_t* n_kept) {
  const size_t state_off = 16, small_bytes = state_off + (size_t)registered_scan_workgroups((uint32_t)n) * 8;
  HIP_TRY(c, st.out.reserve(n * stride + 64));
  HIP_TRY(c, st.small.reserve(small_bytes));
  if (!st.h_kept) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&st.h_kept), 64));
  uint32_t* d_counts = st.small.as<uint32_t>();
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, small_bytes, s));
  launch_registered_scan(d_rec, (uint32_t)n, (uint32_t)stride, pose_from_array(T), st.out.as<uint8_t>(), d_counts,
                         reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), d_counts + 1, s);
  HIP_TRY(c, hipGetLastError());
  // all n records' room rather than a second wait for the count first; the count through a pinned word, as so_icp_transform_cloud's
  if (out) HIP_TRY(c, hipMemcpyAsync(out, st.out.p, n * stride, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st.h_kept, d_counts, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (n_kept) *n_kept = *st.h_kept;
  return SO_ICP_OK;
}

RegisteredScanState* registered_scan_state_of(so_icp_ctx* c) {
  if (!c->rs_state) c->rs_state = std::make_shared<RegisteredScanState>();
  return static_cast<RegisteredScanState*>(c->rs_state.get());
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
  if (const int rc = run_sweep(c, s, st, st.raw.as<uint8_t>(), n, L, width, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, li)) return rc;
  if (const int rc = read_back(c, s, st, li, nodistortion_out, surface_out)) return rc;
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
  const int rc = run_sweep(c, c->stream, st, static_cast<const uint8_t*>(d_raw), width * height, L, width, lidar_start_time, poses, n_poses,
                           poses_are_imu, T_i_l, li);
  if (rc) return rc;
  if (d_nodistortion_out) *d_nodistortion_out = st.rec.p;
  if (d_surface_out) *d_surface_out = st.surf.p;
  if (info) *info = li;
  return SO_ICP_OK;
}

void so_icp_livox_default_layout(so_icp_livox_layout* L) {
  if (!L) return;
  std::memset(L, 0, sizeof(*L));
  // livox_ros_driver2/msg/CustomPoint: uint32 offset_time; float32 x, y, z; uint8 reflectivity, tag, line
  L->point_step = 20;
  L->off_offset_time = 0; L->off_x = 4; L->off_y = 8; L->off_z = 12; L->off_reflectivity = 16; L->off_tag = 17; L->off_line = 18;
  L->n_scans = 4; L->filter_point_size = 3; L->min_range = 0.2f;  // featureExtraction.cpp:120-130
  L->R_imu_laser_gravity[0] = L->R_imu_laser_gravity[4] = L->R_imu_laser_gravity[8] = 1.0;
}

int so_icp_extract_features_livox(so_icp_ctx* c, const void* raw, uint32_t n, const so_icp_livox_layout* L, double lidar_start_time,
                                  const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7],
                                  void* nodistortion_out, void* surface_out, so_icp_feature_info* info) {
  if (const int rc = check_livox_args(c, "so_icp_extract_features_livox", raw, n, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  hipStream_t s = aux_stream(c);  // (host buffers in and out: as so_icp_extract_features)
  if (n) {
    const size_t bytes = livox_payload_bytes(n, L);
    HIP_TRY(c, st.raw.reserve(bytes + 64));
    HIP_TRY(c, hipMemcpyAsync(st.raw.p, raw, bytes, hipMemcpyHostToDevice, s));  // (pageable, straight from the message: see above)
  }
  so_icp_feature_info li;
  if (const int rc = run_livox(c, s, st, st.raw.as<uint8_t>(), n, L, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, li)) return rc;
  if (const int rc = read_back(c, s, st, li, nodistortion_out, surface_out)) return rc;
  if (info) *info = li;
  return SO_ICP_OK;
}

int so_icp_extract_features_livox_dev(so_icp_ctx* c, const void* d_raw, uint32_t n, const so_icp_livox_layout* L, double lidar_start_time,
                                      const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7],
                                      void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_livox_args(c, "so_icp_extract_features_livox_dev", d_raw, n, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  so_icp_feature_info li;
  const int rc = run_livox(c, c->stream, st, static_cast<const uint8_t*>(d_raw), n, L, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, li);
  if (rc) return rc;
  if (d_nodistortion_out) *d_nodistortion_out = st.rec.p;
  if (d_surface_out) *d_surface_out = st.surf.p;
  if (info) *info = li;
  return SO_ICP_OK;
}

int so_icp_extract_features_untimed(so_icp_ctx* c, const void* raw, uint32_t width, uint32_t height, const so_icp_untimed_layout* L,
                                    double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu,
                                    const double T_i_l[7], void* nodistortion_out, void* surface_out, so_icp_feature_info* info) {
  if (const int rc = check_untimed_args(c, "so_icp_extract_features_untimed", raw, width, height, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  hipStream_t s = aux_stream(c);  // (host buffers in and out: as so_icp_extract_features)
  const uint32_t n = width * height;
  if (n) {
    const size_t bytes = (size_t)L->row_step * (height - 1) + (size_t)width * L->point_step;  // (the last row's tail is never read)
    HIP_TRY(c, st.raw.reserve(bytes + 64));
    HIP_TRY(c, hipMemcpyAsync(st.raw.p, raw, bytes, hipMemcpyHostToDevice, s));  // (pageable, straight from the message: see above)
  }
  so_icp_feature_info li;
  if (const int rc = run_untimed(c, s, st, st.raw.as<uint8_t>(), n, L, width, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, li)) return rc;
  if (const int rc = read_back(c, s, st, li, nodistortion_out, surface_out)) return rc;
  if (info) *info = li;
  return SO_ICP_OK;
}

int so_icp_extract_features_untimed_dev(so_icp_ctx* c, const void* d_raw, uint32_t width, uint32_t height, const so_icp_untimed_layout* L,
                                        double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu,
                                        const double T_i_l[7], void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_untimed_args(c, "so_icp_extract_features_untimed_dev", d_raw, width, height, L, poses, n_poses)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  so_icp_feature_info li;
  const int rc = run_untimed(c, c->stream, st, static_cast<const uint8_t*>(d_raw), width * height, L, width, lidar_start_time, poses, n_poses,
                             poses_are_imu, T_i_l, li);
  if (rc) return rc;
  if (d_nodistortion_out) *d_nodistortion_out = st.rec.p;
  if (d_surface_out) *d_surface_out = st.surf.p;
  if (info) *info = li;
  return SO_ICP_OK;
}

// laserMapping::publishTopic's registered scan, laserMapping.cpp:464-493 with utils::pointAssociateToMap, superodom_utils.cpp:148-158
// (kernel: feature_kernels.hip registered_scan_kernel).  The auxiliary queue, as so_icp_transform_cloud: beside the map insert that
// so_icp_localization left in the context's queue.
int so_icp_registered_scan_dev(so_icp_ctx* c, const void* d_records, size_t n, size_t stride, const double T[7], void* out, void** d_out,
                               size_t* n_kept) {
  if (const int rc = check_registered_scan_args(c, d_records, n, stride, T, true)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (n_kept) *n_kept = 0;
  if (d_out) *d_out = nullptr;
  if (!n) return SO_ICP_OK;
  RegisteredScanState& st = *registered_scan_state_of(c);
  if (const int rc = run_registered_scan(c, aux_stream(c), st, static_cast<const uint8_t*>(d_records), n, stride, T, out, n_kept)) return rc;
  if (d_out) *d_out = st.out.p;
  return SO_ICP_OK;
}

int so_icp_registered_scan(so_icp_ctx* c, const void* records, size_t n, size_t stride, const double T[7], void* out, size_t* n_kept) {
  if (const int rc = check_registered_scan_args(c, records, n, stride, T, false)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (n_kept) *n_kept = 0;
  if (!n) return SO_ICP_OK;
  RegisteredScanState& st = *registered_scan_state_of(c);
  hipStream_t s = aux_stream(c);
  HIP_TRY(c, st.in.reserve(n * stride + 64));
  HIP_TRY(c, hipMemcpyAsync(st.in.p, records, n * stride, hipMemcpyHostToDevice, s));
  return run_registered_scan(c, s, st, st.in.as<uint8_t>(), n, stride, T, out, n_kept);
}

}  // extern "C"
