// prefilter.cpp -- so_icp_prefilter_announce / so_icp_prefilter_scan(_dev): laserMapping::adjustVoxelSize (laserMapping.cpp:598-651) on
// the device: cloud statistics -> resolution choice -> pcl::VoxelGrid of the surf cloud at planeRes; the resolutions are pushed into
// the context like the node does.
// The pre-filter as ONE enqueue (prefilter_fast): statistics -> decision and leaf grid on the device (vg_decide_kernel) -> VoxelGrid ->
// one read-back (decision + number of leaves).  A case the device leaves to the host (the statistic within the rounding band of a
// threshold, a leaf grid that overflows int32) goes on with the host-decided sequence: host_statistics, host_decide, host_filter.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "ctx.h"
#include "map_kernels.h"

namespace {

constexpr int kPrefilterHostPath = 1000;  // prefilter_fast: the device left the decision to the host
constexpr int kStatBlocks = 256;          // launch_vg_stats: workgroups, each leaving 10 partial statistics

// One so_icp_prefilter_scan(_dev) call: the cloud in pf_in (n records of sf floats), its queue, what the caller asked for and
// where the result goes
struct Job {
  so_icp_ctx* c; hipStream_t s;
  size_t n, stride_bytes; uint32_t sf;
  int auto_voxel_size; float line_res, plane_res;
  bool announced;  // pf_in is the copy so_icp_prefilter_announce started
  void** d_out; size_t* n_out; so_icp_prefilter_info* info;
};

so_icp_prefilter_info default_info(float line_res, float plane_res) {
  so_icp_prefilter_info li;
  std::memset(&li, 0, sizeof(li));
  li.line_res = line_res; li.plane_res = plane_res;
  return li;
}

// the way out with a cloud of n_out points in pf_out
int done(const Job& j, so_icp_prefilter_info li, size_t n_out) {
  *j.d_out = j.c->pf_out.p; *j.n_out = n_out;
  j.c->pf_inten_n = n_out; j.c->pf_inten_on = j.c->intensity_off >= 0;  // (what so_icp_prefilter_intensity and so_icp_localization_dev go by)
  li.reserved = j.announced ? 1 : 0;
  if (j.info) *j.info = li;
  return SO_ICP_OK;
}

int prefilter_reserve_work(so_icp_ctx* c, size_t n) {
  const size_t cap = n + 1024;
  HIP_TRY(c, c->pf_w.reserve(cap * 16)); HIP_TRY(c, c->pf_s.reserve(cap * 16));
  for (DevBuf* b : {&c->pf_k0, &c->pf_k1, &c->pf_v0, &c->pf_v1, &c->pf_flags, &c->pf_pos, &c->pf_heads}) HIP_TRY(c, b->reserve((cap + 1) * 4));
  if (c->pf_temp_for != cap) { c->pf_temp_need = map_sort_temp_bytes(cap) + 256; c->pf_temp_for = cap; }
  HIP_TRY(c, c->pf_temp.reserve(c->pf_temp_need));
  HIP_TRY(c, c->pf_out.reserve((n + 64) * 12));
  if (c->intensity_off >= 0) HIP_TRY(c, c->pf_inten.reserve((n + 64) * 4));
  return SO_ICP_OK;
}

// the filter's arguments both paths fill alike: the cloud and the work buffers (after prefilter_reserve_work: a reserve may move them)
VoxelFilterArgs filter_args(so_icp_ctx* c, size_t n, uint32_t sf) {
  VoxelFilterArgs a{};
  a.d_xyz = c->pf_in.as<float>(); a.n = (uint32_t)n; a.stride_floats = sf;
  a.wpts = c->pf_w.as<float4>(); a.spts = c->pf_s.as<float4>();
  a.keys0 = c->pf_k0.as<uint32_t>(); a.keys1 = c->pf_k1.as<uint32_t>(); a.vals0 = c->pf_v0.as<uint32_t>(); a.vals1 = c->pf_v1.as<uint32_t>();
  a.flags = c->pf_flags.as<uint32_t>(); a.pos = c->pf_pos.as<uint32_t>(); a.heads = c->pf_heads.as<uint32_t>();
  a.d_out = c->pf_out.as<float>();
  // the intensity column (so_icp_set_cloud_intensity): read out of the records in pf_in, averaged per leaf into an array of its own
  a.d_inten = intensity_in(c, c->pf_in.as<float>(), (size_t)sf * 4); a.inten_stride = sf;
  a.d_out_inten = c->intensity_off >= 0 ? c->pf_inten.as<float>() : nullptr;
  a.temp = c->pf_temp.p; a.temp_bytes = c->pf_temp.cap;
  return a;
}

// decided on the device; kPrefilterHostPath: not decided there
int prefilter_fast(const Job& j, so_icp_prefilter_info li) {
  so_icp_ctx* c = j.c;
  constexpr size_t kDecOff = kVgCounterWords * sizeof(uint32_t), kPartOff = 512;  // (the counters, kVgCnt*, come first)
  static_assert(kDecOff + sizeof(VgDecision) <= kPartOff, "layout of pf_dec");
  constexpr uint32_t kScanRecords = 1024;  // look-back records of the filter's fused scan: 2 048 points each
  constexpr size_t kStateOff = kPartOff + kStatBlocks * 10 * sizeof(double);
  HIP_TRY(c, c->pf_dec.reserve(kStateOff + kScanRecords * sizeof(unsigned long long) + 64));
  if (!c->h_pf) HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->h_pf), sizeof(VgDecision)));
  uint32_t* d_counters = c->pf_dec.as<uint32_t>();
  VgDecision* d_dec = reinterpret_cast<VgDecision*>(c->pf_dec.as<uint8_t>() + kDecOff);
  double* d_part = reinterpret_cast<double*>(c->pf_dec.as<uint8_t>() + kPartOff);
  int rc = prefilter_reserve_work(c, j.n);
  if (rc) return rc;
  VgCandidates cand;
  cand.line_res[0] = 0.1f; cand.plane_res[0] = 0.2f;            // laserMapping.cpp:622-626
  cand.line_res[1] = j.line_res; cand.plane_res[1] = j.plane_res;
  cand.line_res[2] = 0.4f; cand.plane_res[2] = 0.8f;            // :627-631
  for (int k = 0; k < 3; ++k) cand.inv_leaf[k] = 1.0f / cand.plane_res[k];
  launch_vg_stats(c->pf_in.as<float>(), (uint32_t)j.n, j.sf, d_part, kStatBlocks, j.s);
  unsigned long long* d_state = reinterpret_cast<unsigned long long*>(c->pf_dec.as<uint8_t>() + kStateOff);
  launch_vg_decide(d_part, kStatBlocks, (uint32_t)j.n, j.auto_voxel_size, cand, d_dec, d_counters, d_state, kScanRecords, j.s);
  auto a = filter_args(c, j.n, j.sf);
  a.d_decision = d_dec; a.scan_state = d_state; a.n_scan_state = kScanRecords;
  a.d_n_cent = d_counters;
  launch_voxel_filter(a, j.s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(c->h_pf, d_dec, sizeof(VgDecision), hipMemcpyDeviceToHost, j.s));
  HIP_TRY(c, hipStreamSynchronize(j.s));
  const VgDecision& H = *c->h_pf;
  if (H.flags) return kPrefilterHostPath;
  if (j.auto_voxel_size) {
    li.statistic_in_input_order = 0;
    li.average_distance = (double)H.average_distance;
    li.count_far_points = (int32_t)H.acc[3];
    li.increase_blind_radius = li.count_far_points > 3000;
  }
  li.line_res = H.line_res; li.plane_res = H.plane_res;
  rc = so_icp_set_resolution(c, li.line_res, li.plane_res);  // lmap.cpp:648-649
  if (rc) return rc;
  return done(j, li, H.n_leaves);
}

// statistics + bounding box, folded into acc[10]: four sums, three minima, three maxima (fp64 tree sums; the reference accumulates |x|,|y|,|z| in float in input order --
// the statistic only feeds the 25 / 65 thresholds and the 3000-far-points flag)
int host_statistics(const Job& j, double acc[10]) {
  so_icp_ctx* c = j.c;
  HIP_TRY(c, c->pf_small.reserve(kStatBlocks * 10 * sizeof(double) + 128));
  launch_vg_stats(c->pf_in.as<float>(), (uint32_t)j.n, j.sf, c->pf_small.as<double>(), kStatBlocks, j.s);
  std::vector<double> part((size_t)kStatBlocks * 10);
  HIP_TRY(c, hipMemcpyAsync(part.data(), c->pf_small.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, j.s));
  HIP_TRY(c, hipStreamSynchronize(j.s));
  for (int b = 0; b < kStatBlocks; ++b)
    for (int k = 0; k < 10; ++k) {
      const double v = part[(size_t)b * 10 + k];
      acc[k] = k < 4 ? acc[k] + v : (k < 7 ? std::min(acc[k], v) : std::max(acc[k], v));
    }
  return SO_ICP_OK;
}

// adjustVoxelSize's choice of the resolutions from the statistics, pushed into the context
int host_decide(const Job& j, const double acc[10], so_icp_prefilter_info& li) {
  so_icp_ctx* c = j.c;
  const size_t n = j.n;
  if (j.auto_voxel_size) {
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
      launch_vg_stats_inorder(c->pf_in.as<float>(), (uint32_t)n, j.sf, d3, j.s);
      float h3[3] = {0, 0, 0};
      HIP_TRY(c, hipMemcpyAsync(h3, d3, sizeof(h3), hipMemcpyDeviceToHost, j.s));
      HIP_TRY(c, hipStreamSynchronize(j.s));
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
  return so_icp_set_resolution(c, li.line_res, li.plane_res);  // lmap.cpp:648-649
}

// pcl::VoxelGrid::applyFilter: bounding box -> min_b / div_b; "leaf size too small" passes the cloud through
int host_filter(const Job& j, const double acc[10], const so_icp_prefilter_info& li) {
  so_icp_ctx* c = j.c;
  const size_t n = j.n;
  const float leaf = li.plane_res, inv = 1.0f / leaf;
  const float mn[3] = {(float)acc[4], (float)acc[5], (float)acc[6]}, mx[3] = {(float)acc[7], (float)acc[8], (float)acc[9]};
  const int64_t dx = (int64_t)((mx[0] - mn[0]) * inv) + 1, dy = (int64_t)((mx[1] - mn[1]) * inv) + 1, dz = (int64_t)((mx[2] - mn[2]) * inv) + 1;
  HIP_TRY(c, c->pf_out.reserve((n + 64) * 12));
  if (dx * dy * dz > (int64_t)INT32_MAX) {
    if (j.sf == 3) HIP_TRY(c, hipMemcpyAsync(c->pf_out.p, c->pf_in.p, n * 12, hipMemcpyDeviceToDevice, j.s));
    else HIP_TRY(c, hipMemcpy2DAsync(c->pf_out.p, 12, c->pf_in.p, j.stride_bytes, 12, n, hipMemcpyDeviceToDevice, j.s));
    if (c->intensity_off >= 0) {  // the intensities pass through with the points, in input order
      HIP_TRY(c, c->pf_inten.reserve((n + 64) * 4));
      if (const float* src = intensity_in(c, c->pf_in.as<float>(), j.stride_bytes))
        HIP_TRY(c, hipMemcpy2DAsync(c->pf_inten.p, 4, src, j.stride_bytes, 4, n, hipMemcpyDeviceToDevice, j.s));
      else HIP_TRY(c, hipMemsetAsync(c->pf_inten.p, 0, n * 4, j.s));
    }
    HIP_TRY(c, hipStreamSynchronize(j.s));
    return done(j, li, n);
  }
  const int rc = prefilter_reserve_work(c, n);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(c->pf_small.p, 0, kVgCounterWords * sizeof(uint32_t), j.s));
  auto a = filter_args(c, n, j.sf);
  for (int k = 0; k < 3; ++k) {
    a.min_b[k] = (int)std::floor(mn[k] * inv);
    a.div_b[k] = (int)std::floor(mx[k] * inv) - a.min_b[k] + 1;
  }
  a.inv_leaf = inv;
  a.d_n_cent = c->pf_small.as<uint32_t>();
  launch_voxel_filter(a, j.s);
  uint32_t n_leaves = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_leaves, c->pf_small.as<uint32_t>() + kVgCntLeaves, sizeof(uint32_t), hipMemcpyDeviceToHost, j.s));
  HIP_TRY(c, hipStreamSynchronize(j.s));
  return done(j, li, n_leaves);
}

// raw cloud -> pf_in (with its stride) -- unless it was announced (so_icp_prefilter_announce): then its copy went into the queue long
// ago (34 us for a 131 072-point sweep, beside the registration of the frame before) and the two buffers change places
int take_or_upload(Job& j, const float* xyz, bool xyz_on_device) {
  so_icp_ctx* c = j.c;
  if (!xyz_on_device) {
    std::lock_guard<std::mutex> lk(c->pf_mu);
    j.announced = c->pf_announced.on && c->pf_announced.ptr == (const void*)xyz && c->pf_announced.n == j.n && c->pf_announced.stride == j.stride_bytes &&
                  c->pf_stage.p != nullptr;
    c->pf_announced.on = false;  // (taken, or not meant for this call: a copy still in this queue ends before this call's read-back does)
    if (j.announced) std::swap(c->pf_in, c->pf_stage);
  }
  if (!j.announced) {
    HIP_TRY(c, c->pf_in.reserve(j.n * j.stride_bytes + 64));
    HIP_TRY(c, hipMemcpyAsync(c->pf_in.p, xyz, j.n * j.stride_bytes, xyz_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, j.s));
  }
  return SO_ICP_OK;
}

// xyz_on_device: the cloud is already in HBM (so_icp_prefilter_scan_dev) -- one copy on the device into pf_in, and from there the
// host entry's path, so both entries give the same bits
int prefilter_scan_impl(so_icp_ctx* c, const float* xyz, bool xyz_on_device, size_t n, size_t stride_bytes, int auto_voxel_size,
                        float line_res, float plane_res, void** d_out, size_t* n_out, so_icp_prefilter_info* info) {
  if (!c || (!xyz && n) || !d_out || !n_out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (const int rc = normalise_stride(c, &stride_bytes)) return rc;
  // The pre-filter reads the caller's cloud and writes its own buffers: nothing the map insert of the previous frame (still in the
  // context's queue when Localization() returned) touches -- that insert's first kernel, the only reader of the previous filtered
  // cloud, had finished before Localization() returned.  On its own queue it runs beside the insert instead of behind it; the call
  // returns after its own read-back, so the registration that follows finds the filtered cloud complete.
  Job j{c, aux_stream(c), n, stride_bytes, (uint32_t)(stride_bytes / 4), auto_voxel_size, line_res, plane_res, false, d_out, n_out, info};
  so_icp_prefilter_info li = default_info(line_res, plane_res);
  *d_out = nullptr; *n_out = 0;
  c->pf_inten_n = 0; c->pf_inten_on = c->intensity_off >= 0;
  if (!n) { if (info) *info = li; return so_icp_set_resolution(c, line_res, plane_res); }
  int rc = take_or_upload(j, xyz, xyz_on_device);
  if (rc) return rc;
  if (c->pf_fast) {
    rc = prefilter_fast(j, li);
    if (rc != kPrefilterHostPath) return rc;
  }
  double acc[10] = {0, 0, 0, 0, 3.0e38, 3.0e38, 3.0e38, -3.0e38, -3.0e38, -3.0e38};
  rc = host_statistics(j, acc);
  if (!rc) rc = host_decide(j, acc, li);
  return rc ? rc : host_filter(j, acc, li);
}

}  // namespace

extern "C" {

int so_icp_prefilter_announce(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (const int rc = normalise_stride(c, &stride_bytes)) return rc;
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

int so_icp_prefilter_intensity(so_icp_ctx* c, float* out, size_t cap, void** d_out, size_t* n_out) {
  if (!c || !n_out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  *n_out = 0;
  if (d_out) *d_out = nullptr;
  if (!c->pf_inten_on || !c->pf_inten_n) return SO_ICP_OK;  // (the switch was off during the last pre-filter: it kept none)
  const size_t n = c->pf_inten_n;
  if (out) {
    if (cap < n) return fail(c, SO_ICP_E_INVALID, "so_icp_prefilter_intensity: out holds fewer floats than the last pre-filter's output has points");
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    hipStream_t s = aux_stream(c);
    HIP_TRY(c, hipMemcpyAsync(out, c->pf_inten.p, n * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  if (d_out) *d_out = c->pf_inten.p;
  *n_out = n;
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
