// cloud_steps.cpp -- the host-in / host-out steps around Localization(): de-skew (so_icp_deskew_scan(_dev)), the node's registered
// scan (so_icp_transform_cloud) and so_icp_download_scan.
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "ctx.h"
#include "deskew_math.h"
#include "map_kernels.h"

extern "C" {

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

}  // extern "C"
