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
#include <array>
#include <cstring>
#include <functional>
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
  DevBuf small;   // counters (kCounters) | the sampler's look-back words | the ingest's | pose table at a 256-byte boundary
  uint32_t* h_counts = nullptr;  // pinned read-back of the counters
  ~FeatureState() {
    for (DevBuf* b : {&raw, &rec, &surf, &small}) b->release();
    if (h_counts) (void)hipHostFree(h_counts);
  }
};
// the words at the front of FeatureState::small, and what follows them
enum : uint32_t { kCntClamped = 0, kCntSurface = 1, kCntSurfTicket = 2, kCntKept = 4, kCntIngestTicket = 5, kCounters = 8 };
constexpr size_t kSurfStateOff = kCounters * sizeof(uint32_t);

// one field of a point in a layout: byte offset, size, its name in messages, and whether -1 (absent) is allowed
struct Field { int32_t off; uint32_t bytes; const char* name; bool may_be_absent; };

// what every layout has: the sampler's step, the strides (a Livox sweep has no rows: width 0), the fields, the number of points.
// n_scans_fault: the sensor's own complaint about n_scans (nullptr: none), reported in its place behind filter_point_size.
template <typename Fields>
int check_geometry(so_icp_ctx* c, const std::string& w, int32_t filter_point_size, const char* n_scans_fault, uint32_t point_step, uint32_t row_step,
                   uint32_t width, uint64_t n, const Fields& fields) {
  if (filter_point_size < 1) return fail(c, SO_ICP_E_INVALID, w + ": filter_point_size must be >= 1");
  if (n_scans_fault) return fail(c, SO_ICP_E_INVALID, w + n_scans_fault);
  if (point_step == 0) return fail(c, SO_ICP_E_INVALID, w + ": point_step must be > 0");
  if ((uint64_t)row_step < (uint64_t)width * point_step) return fail(c, SO_ICP_E_INVALID, w + ": row_step < width * point_step");
  for (const Field& q : fields) {
    if (q.off < 0 && !q.may_be_absent) return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " must be >= 0 (a CustomPoint has every field)");
    if (q.off < -1 || (q.off >= 0 && (uint64_t)q.off + q.bytes > point_step)) return fail(c, SO_ICP_E_INVALID, w + ": offset of " + q.name + " lies past point_step");
  }
  if (n >= ((uint64_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, w + ": too many points");
  return SO_ICP_OK;
}

// bytes of a row-major payload that are read (the last row's tail is not)
size_t rows_payload_bytes(uint32_t width, uint32_t height, uint32_t point_step, uint32_t row_step) {
  return (uint64_t)width * height ? (size_t)row_step * (height - 1) + (size_t)width * point_step : 0;
}

// what run() hands a kind's ingest: payload, records, the de-skew's arguments, the counters, the ingest's look-back words, the queue
struct IngestArgs {
  const uint8_t* d_raw; uint8_t* d_rec; double t0; const double* d_tab; uint32_t n_poses; const DeskewFrames& f;
  uint32_t* d_counts; unsigned long long* d_state; hipStream_t s;
};

// One kind of sweep, as run() needs it
struct SweepKind {
  uint32_t n;                   // points in the payload
  uint32_t step;                // the sampler's (filter_point_size)
  float min_range;
  size_t payload_bytes;         // of the payload that are read
  uint32_t ingest_state_words;  // look-back words of the ingest's own compaction (0: it writes one record per point)
  bool count_on_device;         // the number of records is known only behind the ingest (ingest_state_words > 0)
  std::function<void(const IngestArgs&)> ingest;  // the sensor's launch_*ingest_deskew
};

// ---- a PointCloud2 sweep with per-point time (laserCloudHandler, :710-766) ----
int check_layout(so_icp_ctx* c, const char* who, uint32_t width, uint32_t height, const so_icp_sweep_layout* L) {
  const std::string w(who);
  if (L->sensor != SO_ICP_SENSOR_VELODYNE && L->sensor != SO_ICP_SENSOR_OUSTER)
    return fail(c, SO_ICP_E_INVALID, w + ": unknown sensor (SO_ICP_SENSOR_VELODYNE or SO_ICP_SENSOR_OUSTER)");
  if (L->is_bigendian) return fail(c, SO_ICP_E_INVALID, w + ": big-endian payloads are not supported");
  const bool ouster = L->sensor == SO_ICP_SENSOR_OUSTER;
  const Field f[] = {{L->off_x, 4, "x", true}, {L->off_y, 4, "y", true}, {L->off_z, 4, "z", true}, {L->off_intensity, 4, "intensity", true},
                     {L->off_time, 4, "time", true}, {ouster ? -1 : L->off_ring, 2, "ring", true}};
  return check_geometry(c, w, L->filter_point_size, nullptr, L->point_step, L->row_step, width, (uint64_t)width * height, f);
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

SweepKind kind_of(const so_icp_sweep_layout* L, uint32_t width, uint32_t height) {
  const uint32_t n = width * height;
  return {n, (uint32_t)L->filter_point_size, L->min_range, rows_payload_bytes(width, height, L->point_step, L->row_step), 0u, false,
          [=](const IngestArgs& a) {
            launch_ingest_deskew(a.d_raw, n, fields_of(L, width), a.d_rec, a.t0, a.d_tab, a.n_poses, a.f, a.d_counts + kCntClamped, a.s);
          }};
}

// ---- a Livox CustomMsg's points (livoxHandler, :794-806): n points in a row, width = n and height = 1 ----
std::array<Field, 7> livox_fields(const so_icp_livox_layout* L) {
  return {{{L->off_offset_time, 4, "offset_time", false}, {L->off_x, 4, "x", false}, {L->off_y, 4, "y", false}, {L->off_z, 4, "z", false},
           {L->off_reflectivity, 1, "reflectivity", false}, {L->off_tag, 1, "tag", false}, {L->off_line, 1, "line", false}}};
}

int check_layout(so_icp_ctx* c, const char* who, uint32_t n, uint32_t, const so_icp_livox_layout* L) {
  const char* scans = L->n_scans < 0 || L->n_scans > 256 ? ": n_scans must lie in 0 .. 256 (line is a uint8)" : nullptr;
  return check_geometry(c, who, L->filter_point_size, scans, L->point_step, 0u, 0u, n, livox_fields(L));
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
  size_t end = 0;
  for (const Field& q : livox_fields(L)) end = std::max(end, (size_t)q.off + q.bytes);
  return n ? (size_t)(n - 1) * L->point_step + end : 0;
}

SweepKind kind_of(const so_icp_livox_layout* L, uint32_t n, uint32_t) {
  return {n, (uint32_t)L->filter_point_size, L->min_range, livox_payload_bytes(n, L), 0u, false,
          [=](const IngestArgs& a) {
            launch_livox_ingest_deskew(a.d_raw, n, livox_fields_of(L), a.d_rec, a.t0, a.d_tab, a.n_poses, a.f, a.d_counts + kCntClamped, a.s);
          }};
}

// ---- a PointCloud2 sweep without per-point time (assignTimeforPointCloud, :646-708) ----
int check_layout(so_icp_ctx* c, const char* who, uint32_t width, uint32_t height, const so_icp_untimed_layout* L) {
  const std::string w(who);
  if (L->is_bigendian) return fail(c, SO_ICP_E_INVALID, w + ": big-endian payloads are not supported");
  bool scans_ok = false;
  for (int32_t v : {4, 16, 32, 64, 128}) scans_ok = scans_ok || L->n_scans == v;  // featureExtraction.cpp:62
  const Field f[] = {{L->off_x, 4, "x", true}, {L->off_y, 4, "y", true}, {L->off_z, 4, "z", true}, {L->off_intensity, 4, "intensity", true}};
  return check_geometry(c, w, L->filter_point_size, scans_ok ? nullptr : ": n_scans must be 4, 16, 32, 64 or 128", L->point_step, L->row_step, width,
                        (uint64_t)width * height, f);
}

UntimedFields untimed_fields_of(const so_icp_untimed_layout* L, uint32_t width) {
  UntimedFields uf;
  uf.point_step = L->point_step; uf.row_step = L->row_step; uf.width = width;
  uf.x = L->off_x; uf.y = L->off_y; uf.z = L->off_z; uf.intensity = L->off_intensity;
  uf.n_scans = (uint32_t)L->n_scans;
  return uf;
}

// The ingest compacts: the number of records is known only on the device, and surf_sample_kernel takes it as a launch argument
SweepKind kind_of(const so_icp_untimed_layout* L, uint32_t width, uint32_t height) {
  const uint32_t n = width * height;
  return {n, (uint32_t)L->filter_point_size, L->min_range, rows_payload_bytes(width, height, L->point_step, L->row_step), untimed_workgroups(n), true,
          [=](const IngestArgs& a) {
            launch_untimed_ingest_deskew(a.d_raw, n, untimed_fields_of(L, width), a.d_rec, a.t0, a.d_tab, a.n_poses, a.f, a.d_counts + kCntClamped,
                                         a.d_counts + kCntKept, a.d_state, a.d_counts + kCntIngestTicket, a.s);
          }};
}

// the argument check of all six entries (Layout: one of the three above); a Livox sweep passes width = n, height = 1
template <typename Layout>
int check_args(so_icp_ctx* c, const char* who, const void* raw, uint32_t width, uint32_t height, const Layout* L, const so_icp_stamped_pose* poses,
               size_t n_poses) {
  if (!c || !L || (!raw && (uint64_t)width * height) || (n_poses && !poses)) return SO_ICP_E_INVALID;
  if (const int rc = check_layout(c, who, width, height, L)) return rc;
  if (n_poses >= ((size_t)1 << 24)) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(who) + ": too many poses");
  NEED_DEVICE(c);
  return SO_ICP_OK;
}

// The whole pass on queue s: counters and look-back words cleared, pose table, ingest + de-skew, the sampler, counts read back (one
// wait).  A kind whose ingest compacts has its counts read back between the two launches (a wait of its own), and the sampler runs
// over the records that remain; n_points, deskewed and the sweep-start pose are then reported only once a record exists.
int run(so_icp_ctx* c, hipStream_t s, FeatureState& st, const uint8_t* d_raw, const SweepKind& k, double t0, const so_icp_stamped_pose* poses,
        size_t n_poses, int imu, const double T_i_l[7], so_icp_feature_info& info) {
  static_assert(sizeof(so_icp_stamped_pose) == kStampedPoseDoubles * sizeof(double), "stamped pose = 8 doubles");
  std::memset(&info, 0, sizeof(info));  // what stays where there is no record: zero counts, no de-skew, the identity
  info.q_w_original_l[3] = 1.0;
  DeskewFrames f{};
  std::vector<double> tab;
  double q_start[4] = {0.0, 0.0, 0.0, 1.0}, t_start[3] = {0.0, 0.0, 0.0};  // the sweep-start pose
  if (n_poses && !deskew_setup(reinterpret_cast<const double*>(poses), n_poses, t0, imu, T_i_l, f, tab, q_start, t_start))
    return fail(c, SO_ICP_E_INVALID, "pose buffer times must increase strictly (the reference keeps them in a std::map)");
  auto report_records = [&](uint32_t n_rec) {
    info.n_points = n_rec;
    info.deskewed = n_poses ? 1 : 0;
    std::memcpy(info.q_w_original_l, q_start, sizeof(q_start));
    std::memcpy(info.t_w_original_l, t_start, sizeof(t_start));
  };
  if (!k.count_on_device) report_records(k.n);
  if (!k.n) return SO_ICP_OK;
  const size_t ingest_state_off = kSurfStateOff + (size_t)surf_workgroups(k.n, k.step) * 8,  // (the sampler's words: for up to n records)
               tab_off = (ingest_state_off + (size_t)k.ingest_state_words * 8 + 255) & ~(size_t)255;
  HIP_TRY(c, st.rec.reserve((size_t)k.n * kFeatureRecordBytes));
  HIP_TRY(c, st.surf.reserve((size_t)(surf_candidates(k.n, k.step) + 1) * kFeatureRecordBytes));
  HIP_TRY(c, st.small.reserve(tab_off + tab.size() * sizeof(double) + 64));
  if (!st.h_counts) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&st.h_counts), 64));
  uint8_t* small = st.small.as<uint8_t>();
  uint32_t *d_counts = st.small.as<uint32_t>(), *h = st.h_counts;
  HIP_TRY(c, hipMemsetAsync(small, 0, tab_off, s));
  if (n_poses) HIP_TRY(c, hipMemcpyAsync(small + tab_off, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  k.ingest({d_raw, st.rec.as<uint8_t>(), t0, reinterpret_cast<const double*>(small + tab_off), (uint32_t)n_poses, f, d_counts,
            reinterpret_cast<unsigned long long*>(small + ingest_state_off), s});
  uint32_t n_rec = k.n, first = kCntClamped;  // first: the first counter the last read-back still has to fetch
  if (k.count_on_device) {
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h, d_counts, kCounters * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));  // (also keeps `tab` alive until its upload has been consumed)
    n_rec = h[kCntKept];
    if (!n_rec) return SO_ICP_OK;
    report_records(n_rec);
    info.n_clamped = h[kCntClamped];
    if (!surf_workgroups(n_rec, k.step)) return SO_ICP_OK;  // one record: no candidate
    first = kCntSurface;
  }
  launch_surf_sample(st.rec.as<uint8_t>(), n_rec, k.step, k.min_range, st.surf.as<uint8_t>(), d_counts + kCntSurface,
                     reinterpret_cast<unsigned long long*>(small + kSurfStateOff), d_counts + kCntSurfTicket, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(h + first, d_counts + first, (kCntSurface + 1 - first) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // (also keeps `tab` alive until its upload has been consumed)
  info.n_clamped = h[kCntClamped];
  info.n_surface = h[kCntSurface];
  return SO_ICP_OK;
}

FeatureState* state_of(so_icp_ctx* c) {
  if (!c->fe_state) c->fe_state = std::make_shared<FeatureState>();
  return static_cast<FeatureState*>(c->fe_state.get());
}

// A host entry behind its argument check: the payload copied in, run(), the clouds copied out into the caller's buffers.
// The auxiliary queue (a host buffer in, host buffers out: the queue of the other steps around Localization()).
int extract_host(so_icp_ctx* c, const SweepKind& k, const void* raw, double t0, const so_icp_stamped_pose* poses, size_t n_poses, int imu,
                 const double T_i_l[7], void* nodistortion_out, void* surface_out, so_icp_feature_info* info) {
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));  // (before the auxiliary queue may be created: on the context's device)
  FeatureState& st = *state_of(c);
  hipStream_t s = aux_stream(c);
  if (k.n) {
    HIP_TRY(c, st.raw.reserve(k.payload_bytes + 64));
    // straight from the caller's buffer, as so_icp_prefilter_scan copies its cloud: a copy into a pinned staging buffer first
    // made the call slower (0.419 against 0.289 ms for the 131 072-point Ouster sweep) -- the runtime already
    // pipelines a pageable copy through its own pinned chunks
    HIP_TRY(c, hipMemcpyAsync(st.raw.p, raw, k.payload_bytes, hipMemcpyHostToDevice, s));
  }
  so_icp_feature_info li;
  if (const int rc = run(c, s, st, st.raw.as<uint8_t>(), k, t0, poses, n_poses, imu, T_i_l, li)) return rc;
  if (li.n_points && nodistortion_out) HIP_TRY(c, hipMemcpyAsync(nodistortion_out, st.rec.p, (size_t)li.n_points * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  if (li.n_surface && surface_out) HIP_TRY(c, hipMemcpyAsync(surface_out, st.surf.p, (size_t)li.n_surface * kFeatureRecordBytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (info) *info = li;
  return SO_ICP_OK;
}

// A resident entry behind its argument check: run() on the caller's device buffer and the context's queue (as so_icp_deskew_scan_dev),
// the two clouds handed out where they lie.
int extract_resident(so_icp_ctx* c, const SweepKind& k, const void* d_raw, double t0, const so_icp_stamped_pose* poses, size_t n_poses, int imu,
                     const double T_i_l[7], void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  FeatureState& st = *state_of(c);
  so_icp_feature_info li;
  if (const int rc = run(c, c->stream, st, static_cast<const uint8_t*>(d_raw), k, t0, poses, n_poses, imu, T_i_l, li)) return rc;
  if (d_nodistortion_out) *d_nodistortion_out = st.rec.p;
  if (d_surface_out) *d_surface_out = st.surf.p;
  if (info) *info = li;
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

}  // namespace

extern "C" {

int so_icp_extract_features(so_icp_ctx* c, const void* raw, uint32_t width, uint32_t height, const so_icp_sweep_layout* L, double lidar_start_time,
                            const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7], void* nodistortion_out,
                            void* surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features", raw, width, height, L, poses, n_poses)) return rc;
  return extract_host(c, kind_of(L, width, height), raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, nodistortion_out, surface_out, info);
}

int so_icp_extract_features_dev(so_icp_ctx* c, const void* d_raw, uint32_t width, uint32_t height, const so_icp_sweep_layout* L,
                                double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7],
                                void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features_dev", d_raw, width, height, L, poses, n_poses)) return rc;
  return extract_resident(c, kind_of(L, width, height), d_raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, d_nodistortion_out, d_surface_out, info);
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
  if (const int rc = check_args(c, "so_icp_extract_features_livox", raw, n, 1u, L, poses, n_poses)) return rc;
  return extract_host(c, kind_of(L, n, 1u), raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, nodistortion_out, surface_out, info);
}

int so_icp_extract_features_livox_dev(so_icp_ctx* c, const void* d_raw, uint32_t n, const so_icp_livox_layout* L, double lidar_start_time,
                                      const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu, const double T_i_l[7],
                                      void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features_livox_dev", d_raw, n, 1u, L, poses, n_poses)) return rc;
  return extract_resident(c, kind_of(L, n, 1u), d_raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, d_nodistortion_out, d_surface_out, info);
}

int so_icp_extract_features_untimed(so_icp_ctx* c, const void* raw, uint32_t width, uint32_t height, const so_icp_untimed_layout* L,
                                    double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu,
                                    const double T_i_l[7], void* nodistortion_out, void* surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features_untimed", raw, width, height, L, poses, n_poses)) return rc;
  return extract_host(c, kind_of(L, width, height), raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, nodistortion_out, surface_out, info);
}

int so_icp_extract_features_untimed_dev(so_icp_ctx* c, const void* d_raw, uint32_t width, uint32_t height, const so_icp_untimed_layout* L,
                                        double lidar_start_time, const so_icp_stamped_pose* poses, size_t n_poses, int poses_are_imu,
                                        const double T_i_l[7], void** d_nodistortion_out, void** d_surface_out, so_icp_feature_info* info) {
  if (const int rc = check_args(c, "so_icp_extract_features_untimed_dev", d_raw, width, height, L, poses, n_poses)) return rc;
  return extract_resident(c, kind_of(L, width, height), d_raw, lidar_start_time, poses, n_poses, poses_are_imu, T_i_l, d_nodistortion_out, d_surface_out, info);
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
