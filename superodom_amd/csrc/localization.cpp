// localization.cpp -- so_icp_localization(_dev): LidarSLAM::Localization (registration, checkMotionThresholds, the map insert); the
// host-in / host-out steps around it: de-skew, so_icp_transform_cloud, so_icp_download_scan, the pre-filter (adjustVoxelSize).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ctx.h"
#include "deskew_math.h"
#include "map_kernels.h"

extern "C" {

int so_icp_localization(so_icp_ctx* c, int initialization, const double T_in[7], const float* xyz, size_t n, size_t stride_bytes,
                        double time_laser_odometry, double pose_out[7], so_icp_stats* st) {
  if (!c || !T_in || !pose_out || (!xyz && n)) return SO_ICP_E_INVALID;
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4) return fail(c, SO_ICP_E_INVALID, "stride_bytes must be a multiple of 4");
  if (!c->host_only) HIP_TRY(c, hipSetDevice(c->cfg.device_id));  // (the caller may sit on another device / thread)
  const size_t sf = stride_bytes / 4;
  auto transform_and_add = [&](const double T[7]) -> int {  // transformAndAddToMap, LidarSlam.cpp:60-80; TransformPoint, superodom_utils.h:119-123
    std::vector<float> w(n * 3);
    for (size_t i = 0; i < n; ++i) {
      double ox, oy, oz;
      quat_rotate<double>(T + 3, (double)xyz[i * sf], (double)xyz[i * sf + 1], (double)xyz[i * sf + 2], ox, oy, oz);
      w[3 * i] = (float)(ox + T[0]); w[3 * i + 1] = (float)(oy + T[1]); w[3 * i + 2] = (float)(oz + T[2]);
    }
    if (c->dmap) { const int r = c->dmap->add_surf_host(w.data(), n, 3, c->err); return r < 0 ? (r == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP) : exchange_map_counts(c); }
    return c->map.add_surf(w.data(), n, 3) < 0 ? fail(c, SO_ICP_E_INVALID, "LocalMap insert failed") : SO_ICP_OK;
  };
  auto transform_and_add_dev = [&](const float* d_scan, const double T[7]) -> int {  // same, entirely on the device
    // (one launch transforms the scan, finds every point's cube and lays the insert round out on the device; the insert is
    //  enqueued without a read-back and -- unless SOICP_MAP_FAST=sync -- completes behind this call: device_map.h, settle)
    if (const int rs = c->dmap->settle(c->err); rs < 0) return rs == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP;  // (before d_world may be re-allocated)
    HIP_TRY(c, c->d_world.reserve((n + 64) * 12));
    const int r = c->dmap->add_scan_dev(d_scan, n, T, c->d_world.as<float>(), c->dmap->defer_enabled() && !c->dmap->sharded(), c->err);
    return r < 0 ? (r == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP) : exchange_map_counts(c);
  };
  if (!initialization) {  // initializeMapping, LidarSlam.cpp:83-94
    std::memcpy(pose_out, T_in, 7 * sizeof(double));
    if (st) std::memset(st, 0, sizeof(*st));
    if (!c->host_only) drop_staged(c, xyz, n, stride_bytes);
    if (c->dmap) c->dmap->set_origin(T_in); else c->map.set_origin(T_in);
    const int r = transform_and_add(T_in);
    if (r) return r;
    c->last_time = time_laser_odometry;
    return SO_ICP_MAP_SEEDED;
  }
  so_icp_stats local;
  if (!st) st = &local;
  NEED_DEVICE(c);
  // (the scan the registration ran on -- staged slot or d_scan_own -- is still resident afterwards: the insert reuses it)
  const float* d_scan = nullptr;
  int rc = resolve_scan(c, xyz, n, stride_bytes, &d_scan);
  if (rc) return rc;
  rc = register_core(c, d_scan, n, T_in, pose_out, st);
  c->scan_staged = false;
  if (rc != SO_ICP_OK) { release_staged(c); return rc; }  // NOT_ENOUGH: the reference returns before the post-processing (LidarSlam.cpp:113-116)
  // checkMotionThresholds, LidarSlam.cpp:173-195: always accepts; only the startupCount side effect survives
  const double dt = time_laser_odometry - c->last_time;
  if (st->translation_from_last / dt > c->cfg.velocity_failure_threshold) c->startup_count = 5;
  st->startup_count = c->startup_count;
  int r;
  if (c->dmap) r = transform_and_add_dev(d_scan, pose_out);  // LidarSlam.cpp:163-167
  else r = transform_and_add(pose_out);
  release_staged(c);
  if (r) return r;
  c->last_time = time_laser_odometry;
  return SO_ICP_OK;
}

// featureExtraction::removePointDistortion, featureExtraction.cpp:223-314 (kernel: map_kernels.hip deskew_kernel)
static int deskew_core(so_icp_ctx* c, hipStream_t s, void* d_points, size_t n, size_t stride, size_t time_off, double t0, const so_icp_stamped_pose* poses,
                       size_t n_poses, int imu, const double T_i_l[7], so_icp_deskew_info* info) {
  static_assert(sizeof(so_icp_stamped_pose) == kStampedPoseDoubles * sizeof(double), "stamped pose = 8 doubles");
  DeskewFrames f;
  std::vector<double> host_tab;
  double q_sensor[4], t_sensor[3];
  if (!deskew_setup(reinterpret_cast<const double*>(poses), n_poses, t0, imu, T_i_l, f, host_tab, q_sensor, t_sensor))
    return fail(c, SO_ICP_E_INVALID, "pose buffer times must increase strictly (the reference keeps them in a std::map)");
  if (info) {
    std::memset(info, 0, sizeof(*info));
    for (int k = 0; k < 4; ++k) info->q_w_original_l[k] = q_sensor[k];
    for (int k = 0; k < 3; ++k) info->t_w_original_l[k] = t_sensor[k];
  }
  if (!n) return SO_ICP_OK;
  HIP_TRY(c, c->pf_small.reserve(host_tab.size() * sizeof(double) + 64));
  HIP_TRY(c, hipMemcpyAsync(c->pf_small.p, host_tab.data(), host_tab.size() * sizeof(double), hipMemcpyHostToDevice, s));
  uint32_t* d_cnt = reinterpret_cast<uint32_t*>(c->pf_small.as<uint8_t>() + host_tab.size() * sizeof(double));
  HIP_TRY(c, hipMemsetAsync(d_cnt, 0, 8, s));
  launch_deskew(static_cast<uint8_t*>(d_points), (uint32_t)n, (uint32_t)stride, (uint32_t)time_off, t0, c->pf_small.as<double>(), (uint32_t)n_poses, f, d_cnt, s);
  HIP_TRY(c, hipGetLastError());
  uint32_t cnt = 0;
  HIP_TRY(c, hipMemcpyAsync(&cnt, d_cnt, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));  // also keeps host_tab alive until the upload has been consumed
  if (info) info->n_clamped = cnt;
  return SO_ICP_OK;
}

static int deskew_check(so_icp_ctx* c, const void* points, size_t n, size_t stride, size_t time_off, const so_icp_stamped_pose* poses, size_t n_poses) {
  if (!c || (!points && n) || !poses || !n_poses) return SO_ICP_E_INVALID;
  if (stride < 16 || stride % 4 || time_off % 4 || time_off < 12 || time_off + 4 > stride)
    return fail(c, SO_ICP_E_INVALID, "records: x y z at 0 4 8, a float time at a 4-byte aligned offset in [12, stride - 4], stride a multiple of 4");
  if (n >= ((size_t)1 << 31) || n_poses >= ((size_t)1 << 24)) return fail(c, SO_ICP_E_UNSUPPORTED, "too many points / poses");
  return SO_ICP_OK;
}

int so_icp_deskew_scan_dev(so_icp_ctx* c, void* d_points, size_t n, size_t stride, size_t time_off, double t0, const so_icp_stamped_pose* poses,
                           size_t n_poses, int imu, const double T_i_l[7], so_icp_deskew_info* info) {
  const int rc = deskew_check(c, d_points, n, stride, time_off, poses, n_poses);
  if (rc) return rc;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  return deskew_core(c, c->stream, d_points, n, stride, time_off, t0, poses, n_poses, imu, T_i_l, info);  // (the caller's device buffer: its queue)
}

int so_icp_deskew_scan(so_icp_ctx* c, void* points, size_t n, size_t stride, size_t time_off, double t0, const so_icp_stamped_pose* poses,
                       size_t n_poses, int imu, const double T_i_l[7], so_icp_deskew_info* info) {
  int rc = deskew_check(c, points, n, stride, time_off, poses, n_poses);
  if (rc) return rc;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  hipStream_t s = aux_stream(c);
  if (n) {
    HIP_TRY(c, c->pf_in.reserve(n * stride + 64));
    HIP_TRY(c, hipMemcpyAsync(c->pf_in.p, points, n * stride, hipMemcpyHostToDevice, s));
  }
  rc = deskew_core(c, s, c->pf_in.p, n, stride, time_off, t0, poses, n_poses, imu, T_i_l, info);
  if (rc || !n) return rc;
  HIP_TRY(c, hipMemcpyAsync(points, c->pf_in.p, n * stride, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return SO_ICP_OK;
}

// laserMapping::publishTopic's registered scan, laserMapping.cpp:464-493 (kernel: map_kernels.hip transform_cloud_kernel)
int so_icp_transform_cloud(so_icp_ctx* c, void* points, size_t n, size_t stride, const double T[7], uint8_t* keep, size_t* n_kept) {
  if (!c || (!points && n) || !T) return SO_ICP_E_INVALID;
  if (stride < 12 || stride % 4) return fail(c, SO_ICP_E_INVALID, "records: float x y z at 0 4 8, stride a multiple of 4");
  if (n >= ((size_t)1 << 31)) return fail(c, SO_ICP_E_UNSUPPORTED, "too many points");
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (n_kept) *n_kept = 0;
  if (!n) return SO_ICP_OK;
  hipStream_t s = aux_stream(c);
  HIP_TRY(c, c->pf_in.reserve(n * stride + 64));
  HIP_TRY(c, c->pf_flags.reserve(n + 64));
  HIP_TRY(c, c->pf_small.reserve(256));
  if (!c->h_pf_kept) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pf_kept), 64));
  HIP_TRY(c, hipMemcpyAsync(c->pf_in.p, points, n * stride, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(c->pf_small.p, 0, 8, s));
  launch_transform_cloud(c->pf_in.as<uint8_t>(), (uint32_t)n, (uint32_t)stride, pose_from_array(T), c->pf_flags.as<uint8_t>(), c->pf_small.as<uint32_t>(), s);
  HIP_TRY(c, hipGetLastError());
  // the records and the count first (the count through a pinned word: a copy to pageable memory is staged and synchronised by the
  // runtime); the flags only when a point was dropped -- points within 0.1 m of the world origin, next to never (lmap.cpp:476) --: a
  // caller's std::vector of flags is pageable memory, and its copy cost as much as the records'
  HIP_TRY(c, hipMemcpyAsync(points, c->pf_in.p, n * stride, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(c->h_pf_kept, c->pf_small.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const uint32_t kept = *c->h_pf_kept;
  if (keep) {
    if (kept == (uint32_t)n) std::memset(keep, 1, n);
    else { HIP_TRY(c, hipMemcpyAsync(keep, c->pf_flags.p, n, hipMemcpyDeviceToHost, s)); HIP_TRY(c, hipStreamSynchronize(s)); }
  }
  if (n_kept) *n_kept = kept;
  return SO_ICP_OK;
}

int so_icp_download_scan(so_icp_ctx* c, const void* d_scan, size_t n, float* out_xyz) {
  if (!c || (!d_scan && n) || (!out_xyz && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (!n) return SO_ICP_OK;
  HIP_TRY(c, hipMemcpyAsync(out_xyz, d_scan, n * 12, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SO_ICP_OK;
}

int so_icp_localization_dev(so_icp_ctx* c, int initialization, const double T_in[7], const void* d_scan, size_t n,
                            double time_laser_odometry, double pose_out[7], so_icp_stats* st) {
  if (!c || !T_in || !pose_out || (!d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (!c->dmap) {  // host-side LocalMap (sharded ranks): the insert needs the points on the host
    std::vector<float> h(n * 3);
    const int rc = so_icp_download_scan(c, d_scan, n, h.data());
    if (rc) return rc;
    return so_icp_localization(c, initialization, T_in, h.data(), n, 12, time_laser_odometry, pose_out, st);
  }
  auto transform_and_add_dev = [&](const double T[7]) -> int {  // transformAndAddToMap (LidarSlam.cpp:60-80) on the device
    if (const int rs = c->dmap->settle(c->err); rs < 0) return rs == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP;
    HIP_TRY(c, c->d_world.reserve((n + 64) * 12));
    const int r = c->dmap->add_scan_dev(static_cast<const float*>(d_scan), n, T, c->d_world.as<float>(), c->dmap->defer_enabled() && !c->dmap->sharded(), c->err);
    return r < 0 ? (r == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP) : exchange_map_counts(c);
  };
  if (!initialization) {  // initializeMapping, LidarSlam.cpp:83-94
    std::memcpy(pose_out, T_in, 7 * sizeof(double));
    if (st) std::memset(st, 0, sizeof(*st));
    c->dmap->set_origin(T_in);
    const int r = transform_and_add_dev(T_in);
    if (r) return r;
    c->last_time = time_laser_odometry;
    return SO_ICP_MAP_SEEDED;
  }
  so_icp_stats local;
  if (!st) st = &local;
  const int rc = register_core(c, static_cast<const float*>(d_scan), n, T_in, pose_out, st);
  if (rc != SO_ICP_OK) return rc;
  const double dt = time_laser_odometry - c->last_time;  // checkMotionThresholds, LidarSlam.cpp:173-195
  if (st->translation_from_last / dt > c->cfg.velocity_failure_threshold) c->startup_count = 5;
  st->startup_count = c->startup_count;
  const int r = transform_and_add_dev(pose_out);  // LidarSlam.cpp:163-167
  if (r) return r;
  c->last_time = time_laser_odometry;
  return SO_ICP_OK;
}

// laserMapping::adjustVoxelSize (laserMapping.cpp:598-651) on the device: cloud statistics -> resolution choice ->
// pcl::VoxelGrid of the surf cloud at planeRes; the resolutions are pushed into the context like the node does.
// The pre-filter as ONE enqueue: statistics -> decision and leaf grid on the device (vg_decide_kernel) -> VoxelGrid -> one
// read-back (decision + number of leaves).  kPrefilterHostPath: a case the device leaves to the host (the statistic within
// the rounding band of a threshold, a leaf grid that overflows int32): the caller goes on with the host-decided sequence.
constexpr int kPrefilterHostPath = 1000;
static int prefilter_reserve_work(so_icp_ctx* c, size_t n) {
  const size_t cap = n + 1024;
  HIP_TRY(c, c->pf_w.reserve(cap * 16)); HIP_TRY(c, c->pf_s.reserve(cap * 16));
  for (DevBuf* b : {&c->pf_k0, &c->pf_k1, &c->pf_v0, &c->pf_v1, &c->pf_flags, &c->pf_pos, &c->pf_heads}) HIP_TRY(c, b->reserve((cap + 1) * 4));
  if (c->pf_temp_for != cap) { c->pf_temp_need = map_sort_temp_bytes(cap) + 256; c->pf_temp_for = cap; }
  HIP_TRY(c, c->pf_temp.reserve(c->pf_temp_need));
  HIP_TRY(c, c->pf_out.reserve((n + 64) * 12));
  return SO_ICP_OK;
}
static int prefilter_fast(so_icp_ctx* c, hipStream_t s, size_t n, uint32_t sf, int auto_voxel_size, float line_res, float plane_res,
                          so_icp_prefilter_info& li, void** d_out, size_t* n_out) {
  constexpr int kStatBlocks = 256;
  constexpr size_t kDecOff = kVgCounterWords * sizeof(uint32_t), kPartOff = 512;  // (the counters, kVgCnt*, come first)
  static_assert(kDecOff + sizeof(VgDecision) <= kPartOff, "layout of pf_dec");
  constexpr uint32_t kScanRecords = 1024;  // look-back records of the filter's fused scan: 2 048 points each
  constexpr size_t kStateOff = kPartOff + kStatBlocks * 10 * sizeof(double);
  HIP_TRY(c, c->pf_dec.reserve(kStateOff + kScanRecords * sizeof(unsigned long long) + 64));
  if (!c->h_pf) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pf), sizeof(VgDecision)));
  uint32_t* d_counters = c->pf_dec.as<uint32_t>();
  VgDecision* d_dec = reinterpret_cast<VgDecision*>(c->pf_dec.as<uint8_t>() + kDecOff);
  double* d_part = reinterpret_cast<double*>(c->pf_dec.as<uint8_t>() + kPartOff);
  int rc = prefilter_reserve_work(c, n);
  if (rc) return rc;
  VgCandidates cand;
  cand.line_res[0] = 0.1f; cand.plane_res[0] = 0.2f;            // laserMapping.cpp:622-626
  cand.line_res[1] = line_res; cand.plane_res[1] = plane_res;
  cand.line_res[2] = 0.4f; cand.plane_res[2] = 0.8f;            // :627-631
  for (int k = 0; k < 3; ++k) cand.inv_leaf[k] = 1.0f / cand.plane_res[k];
  launch_vg_stats(c->pf_in.as<float>(), (uint32_t)n, sf, d_part, kStatBlocks, s);
  unsigned long long* d_state = reinterpret_cast<unsigned long long*>(c->pf_dec.as<uint8_t>() + kStateOff);
  launch_vg_decide(d_part, kStatBlocks, (uint32_t)n, auto_voxel_size, cand, d_dec, d_counters, d_state, kScanRecords, s);
  VoxelFilterArgs a{};
  a.d_decision = d_dec; a.scan_state = d_state; a.n_scan_state = kScanRecords;
  a.d_xyz = c->pf_in.as<float>(); a.n = (uint32_t)n; a.stride_floats = sf;
  a.wpts = c->pf_w.as<float4>(); a.spts = c->pf_s.as<float4>();
  a.keys0 = c->pf_k0.as<uint32_t>(); a.keys1 = c->pf_k1.as<uint32_t>(); a.vals0 = c->pf_v0.as<uint32_t>(); a.vals1 = c->pf_v1.as<uint32_t>();
  a.flags = c->pf_flags.as<uint32_t>(); a.pos = c->pf_pos.as<uint32_t>(); a.heads = c->pf_heads.as<uint32_t>();
  a.d_n_cent = d_counters; a.d_out = c->pf_out.as<float>();
  a.temp = c->pf_temp.p; a.temp_bytes = c->pf_temp.cap;
  launch_voxel_filter(a, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(c->h_pf, d_dec, sizeof(VgDecision), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const VgDecision& H = *c->h_pf;
  if (H.flags) return kPrefilterHostPath;
  if (auto_voxel_size) {
    li.statistic_in_input_order = 0;
    li.average_distance = (double)H.average_distance;
    li.count_far_points = (int32_t)H.acc[3];
    li.increase_blind_radius = li.count_far_points > 3000;
  }
  li.line_res = H.line_res; li.plane_res = H.plane_res;
  rc = so_icp_set_resolution(c, li.line_res, li.plane_res);  // lmap.cpp:648-649
  if (rc) return rc;
  *d_out = c->pf_out.p; *n_out = H.n_leaves;
  return SO_ICP_OK;
}

int so_icp_prefilter_announce(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4) return fail(c, SO_ICP_E_INVALID, "stride_bytes must be a multiple of 4");
  hipStream_t s = aux_stream(c);
  std::lock_guard<std::mutex> lk(c->pf_mu);
  if (!xyz || !n) {  // withdrawn: a copy under way must have left the caller's buffer before the caller reuses it
    if (c->pf_announced.on) HIP_TRY(c, hipStreamSynchronize(s));
    c->pf_announced = so_icp_ctx::PfAnnounced{};
    return SO_ICP_OK;
  }
  // (the pre-filter's queue: whatever still reads pf_stage -- nothing does, a taken buffer became pf_in -- or writes it is in front of this copy)
  HIP_TRY(c, c->pf_stage.reserve(n * stride_bytes + 64));
  HIP_TRY(c, hipMemcpyAsync(c->pf_stage.p, xyz, n * stride_bytes, hipMemcpyHostToDevice, s));
  c->pf_announced.ptr = xyz; c->pf_announced.n = n; c->pf_announced.stride = stride_bytes; c->pf_announced.on = true;
  return SO_ICP_OK;
}

// xyz_on_device: the cloud is already in HBM (so_icp_prefilter_scan_dev) -- one copy on the device into pf_in, and from there the
// host entry's path, so both entries give the same bits
static int prefilter_scan_impl(so_icp_ctx* c, const float* xyz, bool xyz_on_device, size_t n, size_t stride_bytes, int auto_voxel_size,
                               float line_res, float plane_res, void** d_out, size_t* n_out, so_icp_prefilter_info* info) {
  if (!c || (!xyz && n) || !d_out || !n_out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4) return fail(c, SO_ICP_E_INVALID, "stride_bytes must be a multiple of 4");
  const uint32_t sf = (uint32_t)(stride_bytes / 4);
  // The pre-filter reads the caller's cloud and writes its own buffers: nothing the map insert of the previous frame (still in the
  // context's queue when Localization() returned) touches -- that insert's first kernel, the only reader of the previous filtered
  // cloud, had finished before Localization() returned.  On its own queue it runs beside the insert instead of behind it; the call
  // returns after its own read-back, so the registration that follows finds the filtered cloud complete.
  hipStream_t s = aux_stream(c);
  so_icp_prefilter_info li;
  std::memset(&li, 0, sizeof(li));
  li.line_res = line_res; li.plane_res = plane_res;
  *d_out = nullptr; *n_out = 0;
  if (!n) { if (info) *info = li; return so_icp_set_resolution(c, line_res, plane_res); }
  // raw cloud -> device (with its stride) -- unless it was announced (so_icp_prefilter_announce): then its copy went into the queue long
  // ago (34 us for a 131 072-point sweep, beside the registration of the frame before) and the two buffers change places
  bool announced = false;
  if (!xyz_on_device) {
    std::lock_guard<std::mutex> lk(c->pf_mu);
    announced = c->pf_announced.on && c->pf_announced.ptr == (const void*)xyz && c->pf_announced.n == n && c->pf_announced.stride == stride_bytes &&
                c->pf_stage.p != nullptr;
    c->pf_announced.on = false;  // (taken, or not meant for this call: a copy still in this queue ends before this call's read-back does)
    if (announced) std::swap(c->pf_in, c->pf_stage);
  }
  if (!announced) {
    HIP_TRY(c, c->pf_in.reserve(n * stride_bytes + 64));
    HIP_TRY(c, hipMemcpyAsync(c->pf_in.p, xyz, n * stride_bytes, xyz_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s));
  }
  if (c->pf_fast) {
    const int frc = prefilter_fast(c, s, n, sf, auto_voxel_size, line_res, plane_res, li, d_out, n_out);
    if (frc != kPrefilterHostPath) { li.reserved = announced ? 1 : 0; if (frc == SO_ICP_OK && info) *info = li; return frc; }
    std::memset(&li, 0, sizeof(li)); li.line_res = line_res; li.plane_res = plane_res;
  }
  // statistics + bounding box (fp64 tree sums; the reference accumulates |x|,|y|,|z| in float in input order --
  // the statistic only feeds the 25 / 65 thresholds and the 3000-far-points flag)
  constexpr int kStatBlocks = 256;
  HIP_TRY(c, c->pf_small.reserve(kStatBlocks * 10 * sizeof(double) + 128));
  launch_vg_stats(c->pf_in.as<float>(), (uint32_t)n, sf, c->pf_small.as<double>(), kStatBlocks, s);
  std::vector<double> part((size_t)kStatBlocks * 10);
  HIP_TRY(c, hipMemcpyAsync(part.data(), c->pf_small.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  double acc[10] = {0, 0, 0, 0, 3.0e38, 3.0e38, 3.0e38, -3.0e38, -3.0e38, -3.0e38};
  for (int b = 0; b < kStatBlocks; ++b)
    for (int k = 0; k < 10; ++k) {
      const double v = part[(size_t)b * 10 + k];
      acc[k] = k < 4 ? acc[k] + v : (k < 7 ? std::min(acc[k], v) : std::max(acc[k], v));
    }
  if (auto_voxel_size) {
    float ax = (float)(acc[0] / (double)n), ay = (float)(acc[1] / (double)n), az = (float)(acc[2] / (double)n);
    // The reference sums |x|, |y|, |z| in FLOAT in input order (laserMapping.cpp:604-611); the tree sums above are the exact sums
    // to ~1e-16.  A sequential float sum of n non-negative terms is within n 2^-24 of the exact one (relative), so the
    // reference's statistic lies within 3 n 2^-24 (+ the roundings of the divisions and the product) of this one: unless the
    // value is that close to a threshold, the resolution it chooses is decided.  Inside the band the reference's own
    // accumulation is run (one wavefront, ~3 ns per point) and ITS value decides -- and is reported.
    const double stat64 = (acc[0] / (double)n) * (acc[1] / (double)n) * (acc[2] / (double)n);
    const double band = 3.1 * (double)n * 5.9604644775390625e-8 + 1e-6;
    li.statistic_in_input_order = 0;
    if (std::fabs(stat64 - 25.0) <= 25.0 * band || std::fabs(stat64 - 65.0) <= 65.0 * band) {
      float* d3 = reinterpret_cast<float*>(c->pf_small.as<double>() + (size_t)kStatBlocks * 10);
      launch_vg_stats_inorder(c->pf_in.as<float>(), (uint32_t)n, sf, d3, s);
      float h3[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h3, d3, sizeof(h3), hipMemcpyDeviceToHost, s));
      HIP_TRY(c, hipStreamSynchronize(s));
      const float fn = (float)n;  // average /= laserCloudSurfLast->points.size()  (Eigen: the scalar becomes a float, one division per axis)
      ax = h3[0] / fn; ay = h3[1] / fn; az = h3[2] / fn;
      li.statistic_in_input_order = 1;
    }
    li.average_distance = (double)(ax * ay * az);       // laserMapping.cpp:620-621 (float product)
    li.count_far_points = (int32_t)acc[3];
    li.increase_blind_radius = li.count_far_points > 3000;
    if (li.average_distance < 25) { li.line_res = 0.1f; li.plane_res = 0.2f; }
    else if (li.average_distance > 65) { li.line_res = 0.4f; li.plane_res = 0.8f; }
  }
  int rc = so_icp_set_resolution(c, li.line_res, li.plane_res);  // lmap.cpp:648-649
  if (rc) return rc;
  // pcl::VoxelGrid::applyFilter: bounding box -> min_b / div_b; "leaf size too small" passes the cloud through
  const float leaf = li.plane_res, inv = 1.0f / leaf;
  const float mn[3] = {(float)acc[4], (float)acc[5], (float)acc[6]}, mx[3] = {(float)acc[7], (float)acc[8], (float)acc[9]};
  const int64_t dx = (int64_t)((mx[0] - mn[0]) * inv) + 1, dy = (int64_t)((mx[1] - mn[1]) * inv) + 1, dz = (int64_t)((mx[2] - mn[2]) * inv) + 1;
  HIP_TRY(c, c->pf_out.reserve((n + 64) * 12));
  if (dx * dy * dz > (int64_t)INT32_MAX) {
    if (sf == 3) HIP_TRY(c, hipMemcpyAsync(c->pf_out.p, c->pf_in.p, n * 12, hipMemcpyDeviceToDevice, s));
    else HIP_TRY(c, hipMemcpy2DAsync(c->pf_out.p, 12, c->pf_in.p, stride_bytes, 12, n, hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    *d_out = c->pf_out.p; *n_out = n;
    li.reserved = announced ? 1 : 0;
    if (info) *info = li;
    return SO_ICP_OK;
  }
  VoxelFilterArgs a{};
  for (int k = 0; k < 3; ++k) {
    a.min_b[k] = (int)std::floor(mn[k] * inv);
    a.div_b[k] = (int)std::floor(mx[k] * inv) - a.min_b[k] + 1;
  }
  const size_t cap = n + 1024;
  HIP_TRY(c, c->pf_w.reserve(cap * 16)); HIP_TRY(c, c->pf_s.reserve(cap * 16));
  for (DevBuf* b : {&c->pf_k0, &c->pf_k1, &c->pf_v0, &c->pf_v1, &c->pf_flags, &c->pf_pos, &c->pf_heads}) HIP_TRY(c, b->reserve((cap + 1) * 4));
  const size_t tb = map_sort_temp_bytes(cap) + 256;
  HIP_TRY(c, c->pf_temp.reserve(tb));
  HIP_TRY(c, hipMemsetAsync(c->pf_small.p, 0, kVgCounterWords * sizeof(uint32_t), s));
  a.d_xyz = c->pf_in.as<float>(); a.n = (uint32_t)n; a.stride_floats = sf; a.inv_leaf = inv;
  a.wpts = c->pf_w.as<float4>(); a.spts = c->pf_s.as<float4>();
  a.keys0 = c->pf_k0.as<uint32_t>(); a.keys1 = c->pf_k1.as<uint32_t>(); a.vals0 = c->pf_v0.as<uint32_t>(); a.vals1 = c->pf_v1.as<uint32_t>();
  a.flags = c->pf_flags.as<uint32_t>(); a.pos = c->pf_pos.as<uint32_t>(); a.heads = c->pf_heads.as<uint32_t>();
  a.d_n_cent = c->pf_small.as<uint32_t>(); a.d_out = c->pf_out.as<float>();
  a.temp = c->pf_temp.p; a.temp_bytes = c->pf_temp.cap;
  launch_voxel_filter(a, s);
  uint32_t n_leaves = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_leaves, c->pf_small.as<uint32_t>() + kVgCntLeaves, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  *d_out = c->pf_out.p; *n_out = n_leaves;
  li.reserved = announced ? 1 : 0;
  if (info) *info = li;
  return SO_ICP_OK;
}

int so_icp_prefilter_scan(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, int auto_voxel_size, float line_res,
                          float plane_res, void** d_out, size_t* n_out, so_icp_prefilter_info* info) {
  return prefilter_scan_impl(c, xyz, false, n, stride_bytes, auto_voxel_size, line_res, plane_res, d_out, n_out, info);
}

int so_icp_prefilter_scan_dev(so_icp_ctx* c, const void* d_xyz, size_t n, size_t stride_bytes, int auto_voxel_size, float line_res,
                              float plane_res, void** d_out, size_t* n_out, so_icp_prefilter_info* info) {
  return prefilter_scan_impl(c, static_cast<const float*>(d_xyz), true, n, stride_bytes, auto_voxel_size, line_res, plane_res, d_out, n_out, info);
}

}  // extern "C"
