// correspondences.cpp -- so_icp_keep_correspondences and so_icp_correspondences: the correspondence set of the last registration
// (the reference's features_corres, LidarSlam.h:209-222) read where the registration left it.  The registration entries keep a packed
// copy of their scan and a small record of what they ran (keep_scan_copy, note_correspondences) while the switch is on; the export is
// one launch of corr_kernels.hip's kernel on the context's queue.
// so_icp_match(_dev) forms such a set at a pose of the caller's without solving (a registration of one outer iteration and no LM
// iteration, so_icp_ctx::match_only); so_icp_correspondence_sums sums the kept set at up to 64 poses on the device
// (corr_sums_kernels.hip).  Together: the matching half and the per-step evaluation of a solver the caller keeps.
// so_icp_keep_correspondence_geometry and so_icp_correspondence_geometry: the neighbours, PCA and observability labels of the kept set.
// The registration entries snapshot what the last fit pass read (keep_neighbour_snapshot, note_correspondence_geometry) while that
// switch is on; the export refits from the snapshot (corr_geometry_kernels.hip).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>

#include "corr_kernels.h"
#include "ctx.h"

namespace soicp::host {

int keep_scan_copy(so_icp_ctx* c, const float* d_scan, size_t n) {
  if (!n) return SO_ICP_OK;
  HIP_TRY(c, c->corr_scan.reserve(n * 12 + 64));
  HIP_TRY(c, hipMemcpyAsync(c->corr_scan.p, d_scan, n * 12, hipMemcpyDeviceToDevice, c->stream));
  return SO_ICP_OK;
}

void note_correspondences(so_icp_ctx* c, const DevState& H, const double guess[7], size_t n, const EvalParams& ep) {
  fill_correspondence_record(c->corr_last, H, guess, n, ep);
}

void fill_correspondence_record(so_icp_ctx::CorrLast& L, const DevState& H, const double guess[7], size_t n, const EvalParams& ep) {
  const int n_it = std::min(H.n_iterations, (int)SO_ICP_MAX_OUTER);
  L.n = n; L.n_accepted = n_it < 1 ? 0u : (uint32_t)H.iters[n_it - 1].num_surf;
  L.a2 = ep.a2; L.variant = ep.variant;
  L.outer_iteration = n_it - 1;
  // (a registration without an outer iteration formed nothing: both poses are its guess)
  std::memcpy(L.pose_fit, n_it <= 1 ? guess : H.iters[n_it - 2].pose_after, sizeof(L.pose_fit));
  std::memcpy(L.pose_eval, n_it < 1 ? guess : H.iters[n_it - 1].pose_after, sizeof(L.pose_eval));
  // (the histograms of the iteration that formed the set: LmSums::hist of so_icp_correspondence_sums; host memory only)
  for (int h = 0; h < 16; ++h) L.hist[h] = n_it < 1 ? 0 : (h < 7 ? H.iters[n_it - 1].reject_hist[h] : H.iters[n_it - 1].obs_hist[h - 7]);
  L.geometry = false;  // (note_correspondence_geometry, behind this call, says otherwise)
  L.valid = true;
}

}  // namespace soicp::host

namespace {

// so_icp_correspondence_geometry: the snapshot the registration entries write, and the export's own buffers (no other entry writes
// those, and the export writes no other entry's buffers)
struct CorrGeomState {
  DevBuf snap_status, snap_idx, snap_pts;  // NeighbourSnapshot, indexed like the scan
  DevBuf records, labels, refit;
  DevBuf small;                // {n_accepted, ticket, refits not accepted, -} | obs_hist[9] + 3 | look-back words of the compaction
  PinnedBuf h_small;           // read-back of the counters and the histogram
  ~CorrGeomState() {
    for (DevBuf* b : {&snap_status, &snap_idx, &snap_pts, &records, &labels, &refit, &small}) b->release();
  }
  NeighbourSnapshot snapshot() const { return NeighbourSnapshot{snap_status.as<uint8_t>(), snap_idx.as<uint32_t>(), snap_pts.as<float>()}; }
};
constexpr size_t kGeomHistOff = 16, kGeomStateOff = 64;  // CorrGeomState::small

CorrGeomState* geometry_state_of(so_icp_ctx* c) {
  if (!c->corr_geom_state) c->corr_geom_state = std::make_shared<CorrGeomState>();
  return static_cast<CorrGeomState*>(c->corr_geom_state.get());
}

}  // namespace

namespace soicp::host {

int keep_neighbour_snapshot(so_icp_ctx* c, size_t n) {
  if (!n) return SO_ICP_OK;
  CorrGeomState& g = *geometry_state_of(c);
  HIP_TRY(c, g.snap_status.reserve(n + 64));
  HIP_TRY(c, g.snap_idx.reserve(n * 20 + 64));
  HIP_TRY(c, g.snap_pts.reserve(n * 60 + 64));
  // (canonical indices: positions in the host-built map, or slot * kCapPerSlot + position in the device map's pool)
  const uint64_t map_extent = c->dmap ? (uint64_t)c->view.n_slots * kCapPerSlot : (uint64_t)c->view.n_points;
  launch_neighbour_snapshot(c->d_status.as<uint8_t>(), c->d_nbr5.as<uint32_t>(), c->view.pts, (uint32_t)std::min<uint64_t>(map_extent, 0xFFFFFFFFull), (uint32_t)n,
                            g.snapshot(), c->stream);
  HIP_TRY(c, hipGetLastError());
  return SO_ICP_OK;
}

void note_correspondence_geometry(so_icp_ctx* c, const MatchParams& mp) {
  so_icp_ctx::CorrLast& L = c->corr_last;
  L.sq_max_dist_f = mp.sq_max_dist_f; L.max_point_dist = mp.max_point_dist;
  L.geometry = true;
}

}  // namespace soicp::host

namespace {

// One launch of the export kernel on the kept set and its snapshot `snap`, into the buffers of `g`; the counters and the histogram
// are in g.h_small when it returns.  `records`, `labels_out`, `refit_out`: host destinations, each nullable
int run_geometry_export(so_icp_ctx* c, const NeighbourSnapshot& snap, CorrGeomState& g, const char* entry, void* records, uint8_t* labels_out,
                        double* refit_out) {
  const so_icp_ctx::CorrLast& L = c->corr_last;
  const size_t n = L.n;
  const size_t nblk = correspondence_workgroups((uint32_t)n), small_bytes = kGeomStateOff + nblk * 8;
  HIP_TRY(c, g.records.reserve(n * kCorrGeomRecordBytes + 64));
  HIP_TRY(c, g.labels.reserve(n * 3 + 64));
  if (refit_out) HIP_TRY(c, g.refit.reserve(n * kCorrRefitBytes + 64));
  HIP_TRY(c, g.small.reserve(small_bytes));
  HIP_TRY(c, g.h_small.reserve(kGeomStateOff));
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemsetAsync(g.small.p, 0, small_bytes, s));
  CorrGeomIn in;
  in.scan = c->corr_scan.as<float>();
  in.snap = snap;
  in.n = (uint32_t)n; in.pose_fit = pose_from_array(L.pose_fit); in.sq_max_dist_f = L.sq_max_dist_f; in.max_point_dist = L.max_point_dist;
  launch_correspondence_geometry(in, g.records.as<uint8_t>(), g.labels.as<uint8_t>(), refit_out ? g.refit.as<double>() : nullptr, g.small.as<uint32_t>(),
                                 reinterpret_cast<int32_t*>(g.small.as<uint8_t>() + kGeomHistOff),
                                 reinterpret_cast<unsigned long long*>(g.small.as<uint8_t>() + kGeomStateOff), s);
  HIP_TRY(c, hipGetLastError());
  // (sized by what the registration counted, as so_icp_correspondences' copy is; the kernel's own count is checked afterwards)
  if (records && L.n_accepted) HIP_TRY(c, hipMemcpyAsync(records, g.records.p, (size_t)L.n_accepted * kCorrGeomRecordBytes, hipMemcpyDeviceToHost, s));
  if (refit_out && L.n_accepted) HIP_TRY(c, hipMemcpyAsync(refit_out, g.refit.p, (size_t)L.n_accepted * kCorrRefitBytes, hipMemcpyDeviceToHost, s));
  if (labels_out) HIP_TRY(c, hipMemcpyAsync(labels_out, g.labels.p, n * 3, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(g.h_small.p, g.small.p, kGeomStateOff, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  uint32_t counts[4];
  std::memcpy(counts, g.h_small.p, sizeof(counts));
  if (counts[0] != L.n_accepted)
    return fail(c, SO_ICP_E_HIP, std::string(entry) + ": the snapshot holds another number of accepted points than the registration reported");
  if (counts[2]) return fail(c, SO_ICP_E_HIP, std::string(entry) + ": the refit rejected a point the registration accepted");
  return SO_ICP_OK;
}

// The export's own buffers: nothing here is written by another entry, and the export writes no other entry's buffers
struct CorrExportState {
  DevBuf records, status, residual;
  DevBuf small;              // {n_accepted, ticket, -, -} | tile sums of the cost | look-back words of the compaction
  PinnedBuf h_small;         // read-back of the counters and the tile sums
  ~CorrExportState() {
    for (DevBuf* b : {&records, &status, &residual, &small}) b->release();
  }
};

CorrExportState* export_state_of(so_icp_ctx* c) {
  if (!c->corr_state) c->corr_state = std::make_shared<CorrExportState>();
  return static_cast<CorrExportState*>(c->corr_state.get());
}

// so_icp_correspondence_sums' own buffers
struct CorrSumsState {
  DevBuf poses, partials, sums;  // the pose table | one partial vector per (tile, pose) | n_poses LmSums
  PinnedBuf h_io;                // the poses on their way in, the sums on their way out
  ~CorrSumsState() {
    for (DevBuf* b : {&poses, &partials, &sums}) b->release();
  }
};

CorrSumsState* sums_state_of(so_icp_ctx* c) {
  if (!c->corr_sums_state) c->corr_sums_state = std::make_shared<CorrSumsState>();
  return static_cast<CorrSumsState*>(c->corr_sums_state.get());
}

// so_icp_match(_dev) behind the argument checks: the registration's own path with so_icp_ctx::match_only set
int match_core(so_icp_ctx* c, const float* d_scan, size_t n, const double pose[7], so_icp_stats* st) {
  double pose_out[7];
  c->scan_staged = false;  // (the scan is the caller's or the context's own upload: no stage slot is consulted or released)
  c->match_only = true;
  const int rc = register_core(c, d_scan, n, pose, pose_out, st);
  c->match_only = false;
  return rc;
}
int match_refusal(so_icp_ctx* c, const char* entry) {
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(entry) + ": a sharded context (world_size > 1) keeps its correspondences per rank");
  if (!c->corr_keep)
    return fail(c, SO_ICP_E_INVALID, std::string(entry) + ": the match leaves its result as the kept correspondence set -- turn it on first with so_icp_keep_correspondences(ctx, 1)");
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_keep_correspondences(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_keep_correspondences: a sharded context (world_size > 1) keeps its correspondences per rank");
  c->corr_keep = on != 0;
  if (!c->corr_keep) { c->corr_last.valid = false; c->corr_geom_keep = false; }
  return SO_ICP_OK;
}

int so_icp_keep_correspondence_geometry(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_keep_correspondence_geometry: a sharded context (world_size > 1) keeps its correspondences per rank");
  if (on && !c->corr_keep)
    return fail(c, SO_ICP_E_INVALID, "so_icp_keep_correspondence_geometry: the geometry belongs to the kept correspondence set -- turn that on first with so_icp_keep_correspondences(ctx, 1)");
  c->corr_geom_keep = on != 0;
  return SO_ICP_OK;
}

int so_icp_correspondence_geometry(so_icp_ctx* c, so_icp_correspondence_geometry_record* records, size_t cap_records, uint8_t* labels_out,
                                   size_t cap_points, void** d_records_out, so_icp_correspondence_geometry_info* info) {
  static_assert(sizeof(so_icp_correspondence_geometry_record) == kCorrGeomRecordBytes, "the kernel writes so_icp_correspondence_geometry_record records");
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  so_icp_correspondence_geometry_info local;
  if (!info) info = &local;
  std::memset(info, 0, sizeof(*info));
  const so_icp_ctx::CorrLast& L = c->corr_last;
  if (!c->corr_keep || !c->corr_geom_keep || !L.valid || !L.geometry) return SO_ICP_OK;
  const size_t n = L.n;
  if (n >= ((size_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_correspondence_geometry: too many points");
  if (labels_out && cap_points < n)
    return fail(c, SO_ICP_E_INVALID, "so_icp_correspondence_geometry: labels_out needs cap_points >= the points of the registered scan");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  info->valid = 1; info->n_points = n; info->outer_iteration = L.outer_iteration;
  std::memcpy(info->pose_fit, L.pose_fit, sizeof(info->pose_fit));
  if (d_records_out) *d_records_out = nullptr;
  if (!n) return SO_ICP_OK;
  CorrGeomState& g = *geometry_state_of(c);
  const bool want_records = records && cap_records >= L.n_accepted;
  if (const int rc = run_geometry_export(c, g.snapshot(), g, "so_icp_correspondence_geometry", want_records ? records : nullptr, labels_out, nullptr)) return rc;
  info->n_accepted = L.n_accepted;
  std::memcpy(info->obs_hist, g.h_small.p + kGeomHistOff, sizeof(info->obs_hist));
  if (d_records_out) *d_records_out = g.records.p;
  return SO_ICP_OK;
}

int so_icp_debug_correspondence_refit(so_icp_ctx* c, double* out, size_t cap, size_t* n_out) {
  if (!c || !n_out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  *n_out = 0;
  const so_icp_ctx::CorrLast& L = c->corr_last;
  if (!c->corr_keep || !c->corr_geom_keep || !L.valid || !L.geometry || !L.n) return SO_ICP_OK;
  if (!out || cap < L.n_accepted) return fail(c, SO_ICP_E_INVALID, "so_icp_debug_correspondence_refit: out needs room for five doubles per accepted point");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  // (buffers of its own, released when it returns: the records of the last so_icp_correspondence_geometry call stay as they are)
  CorrGeomState scratch;
  if (const int rc = run_geometry_export(c, geometry_state_of(c)->snapshot(), scratch, "so_icp_debug_correspondence_refit", nullptr, nullptr, out)) return rc;
  *n_out = L.n_accepted;
  return SO_ICP_OK;
}

int so_icp_correspondences(so_icp_ctx* c, const double pose[7], so_icp_correspondence* records, size_t cap_records, uint8_t* status_out,
                           float* residual_out, size_t cap_points, void** d_records_out, so_icp_correspondence_info* info) {
  static_assert(sizeof(so_icp_correspondence) == kCorrRecordBytes, "the kernel writes so_icp_correspondence records");
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  so_icp_correspondence_info local;
  if (!info) info = &local;
  std::memset(info, 0, sizeof(*info));
  const so_icp_ctx::CorrLast& L = c->corr_last;
  if (!c->corr_keep || !L.valid) return SO_ICP_OK;
  const size_t n = L.n;
  if (n >= ((size_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_correspondences: too many points");
  if ((status_out || residual_out) && cap_points < n)
    return fail(c, SO_ICP_E_INVALID, "so_icp_correspondences: the per-point outputs need cap_points >= the points of the registered scan");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  info->valid = 1; info->n_points = n; info->outer_iteration = L.outer_iteration;
  std::memcpy(info->pose_fit, L.pose_fit, sizeof(info->pose_fit));
  std::memcpy(info->pose_eval, pose ? pose : L.pose_eval, sizeof(info->pose_eval));
  CorrExportState& st = *export_state_of(c);
  if (d_records_out) *d_records_out = nullptr;
  if (!n) return SO_ICP_OK;
  const size_t nblk = correspondence_workgroups((uint32_t)n), cost_off = 16, state_off = cost_off + nblk * 8, small_bytes = state_off + nblk * 8;
  HIP_TRY(c, st.records.reserve(n * kCorrRecordBytes + 64));
  HIP_TRY(c, st.status.reserve(n + 64));
  HIP_TRY(c, st.residual.reserve(n * 4 + 64));
  HIP_TRY(c, st.small.reserve(small_bytes));
  HIP_TRY(c, st.h_small.reserve(state_off));
  hipStream_t s = c->stream;
  uint32_t* d_counts = st.small.as<uint32_t>();
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, small_bytes, s));
  CorrExportIn in;
  in.scan = c->corr_scan.as<float>();
  in.corr = CorrBuffers{c->d_nd.as<double4>(), c->d_coeff.as<double>(), c->d_status.as<uint8_t>()};
  in.n = (uint32_t)n; in.pose = pose_from_array(info->pose_eval); in.a2 = L.a2; in.variant = L.variant;
  launch_correspondences(in, st.records.as<uint8_t>(), st.status.as<uint8_t>(), st.residual.as<float>(), d_counts,
                         reinterpret_cast<double*>(st.small.as<uint8_t>() + cost_off),
                         reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), d_counts + 1, s);
  HIP_TRY(c, hipGetLastError());
  // The number of records is what the registration counted (iterations[last].num_surf_from_scan): the copy is sized by it rather than
  // by a second wait for the kernel's own count, which is checked against it afterwards
  const bool want_records = records && cap_records >= L.n_accepted;
  if (want_records && L.n_accepted) HIP_TRY(c, hipMemcpyAsync(records, st.records.p, (size_t)L.n_accepted * kCorrRecordBytes, hipMemcpyDeviceToHost, s));
  if (status_out) HIP_TRY(c, hipMemcpyAsync(status_out, st.status.p, n, hipMemcpyDeviceToHost, s));
  if (residual_out) HIP_TRY(c, hipMemcpyAsync(residual_out, st.residual.p, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st.h_small.p, st.small.p, state_off, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  uint32_t n_accepted;
  std::memcpy(&n_accepted, st.h_small.p, 4);
  if (n_accepted != L.n_accepted)
    return fail(c, SO_ICP_E_HIP, "so_icp_correspondences: the status bytes hold another number of accepted points than the registration reported");
  double cost = 0;  // the tiles in tile order
  for (size_t b = 0; b < nblk; ++b) { double t; std::memcpy(&t, st.h_small.p + cost_off + b * 8, 8); cost += t; }
  info->n_accepted = n_accepted; info->cost = cost;
  if (d_records_out) *d_records_out = st.records.p;
  return SO_ICP_OK;
}

int so_icp_match_dev(so_icp_ctx* c, const void* d_scan, size_t n, const double pose[7], so_icp_stats* st) {
  if (!c || !pose || (!d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (const int rc = match_refusal(c, "so_icp_match_dev")) return rc;
  if (const int rc = refuse_pending(c, "so_icp_match_dev", kPriorsNone)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  c->corr_last.valid = false;
  return match_core(c, static_cast<const float*>(d_scan), n, pose, st);
}

int so_icp_match(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, const double pose[7], so_icp_stats* st) {
  if (!c || !pose || (!xyz && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (const int rc = match_refusal(c, "so_icp_match")) return rc;
  if (const int rc = refuse_pending(c, "so_icp_match", kPriorsNone)) return rc;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  c->corr_last.valid = false;
  // a plain upload into the context's own scan buffer: a copy of this scan announced with so_icp_stage_scan stays in its slot for the
  // registration it was announced for (the launches that read the upload have completed when the match has reported)
  if (const int rc = upload_scan_impl(c, xyz, n, stride_bytes, c->d_scan_own, /*wait=*/false)) return rc;
  return match_core(c, c->d_scan_own.as<float>(), n, pose, st);
}

int so_icp_correspondence_sums(so_icp_ctx* c, const double* poses, int n_poses, so_icp_sums* sums_out) {
  static_assert(SO_ICP_SUMS_MAX_POSES == kCorrSumsMaxPoses, "the pose table of correspondence_sums_kernel");
  if (!c) return SO_ICP_E_INVALID;
  if (!poses || !sums_out) return fail(c, SO_ICP_E_INVALID, "so_icp_correspondence_sums: poses and sums_out must not be NULL");
  if (n_poses < 1 || n_poses > SO_ICP_SUMS_MAX_POSES) return fail(c, SO_ICP_E_INVALID, "so_icp_correspondence_sums: n_poses must be 1 .. SO_ICP_SUMS_MAX_POSES");
  NEED_DEVICE(c);
  std::memset(sums_out, 0, (size_t)n_poses * sizeof(so_icp_sums));
  const so_icp_ctx::CorrLast& L = c->corr_last;
  if (!c->corr_keep || !L.valid) return SO_ICP_OK;
  CorrSumsHist hist;
  for (int h = 0; h < 16; ++h) hist.v[h] = (double)L.hist[h];
  const size_t n = L.n;
  if (!n) {  // a kept set of no points: zero sums, its histograms
    for (int k = 0; k < n_poses; ++k) std::memcpy(sums_out[k].hist, hist.v, sizeof(hist.v));
    return SO_ICP_OK;
  }
  if (n >= ((size_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_correspondence_sums: too many points");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  CorrSumsState& st = *sums_state_of(c);
  const size_t nblk = correspondence_workgroups((uint32_t)n), pose_bytes = (size_t)n_poses * 7 * sizeof(double), sums_bytes = (size_t)n_poses * sizeof(so_icp_sums);
  HIP_TRY(c, st.h_io.reserve((size_t)SO_ICP_SUMS_MAX_POSES * sizeof(so_icp_sums)));
  HIP_TRY(c, st.poses.reserve((size_t)SO_ICP_SUMS_MAX_POSES * 7 * sizeof(double)));
  HIP_TRY(c, st.sums.reserve((size_t)SO_ICP_SUMS_MAX_POSES * sizeof(so_icp_sums)));
  HIP_TRY(c, st.partials.reserve(nblk * (size_t)n_poses * kCorrSumsAcc * sizeof(double)));
  hipStream_t s = c->stream;
  // (the poses go through pinned memory: the copy is then asynchronous whatever the caller's buffer is, and the caller's is free at once)
  std::memcpy(st.h_io.p, poses, pose_bytes);
  HIP_TRY(c, hipMemcpyAsync(st.poses.p, st.h_io.p, pose_bytes, hipMemcpyHostToDevice, s));
  CorrSumsIn in;
  in.scan = c->corr_scan.as<float>();
  in.corr = CorrBuffers{c->d_nd.as<double4>(), c->d_coeff.as<double>(), c->d_status.as<uint8_t>()};
  in.n = (uint32_t)n; in.a2 = L.a2; in.variant = L.variant;
  launch_correspondence_sums(in, st.poses.as<double>(), (uint32_t)n_poses, hist, st.partials.as<double>(), st.sums.as<double>(), s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_io.p, st.sums.p, sums_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  std::memcpy(sums_out, st.h_io.p, sums_bytes);
  for (int k = 0; k < n_poses; ++k)
    if (sums_out[k].count != (double)L.n_accepted)
      return fail(c, SO_ICP_E_HIP, "so_icp_correspondence_sums: the status bytes hold another number of accepted points than the registration reported");
  return SO_ICP_OK;
}

}  // extern "C"
