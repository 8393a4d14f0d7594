// corr_geometry_kernels.hip -- the geometry of a registration's plane correspondences (so_icp_correspondence_geometry): what the
// reference keeps of pcaFeature inside OptimizationParameter (LidarSlam.h:209-222) and what FeatureObservabilityAnalysis
// (LidarSlam.cpp:574-693) labels, as one record per ACCEPTED scan point, in scan order, pairing with so_icp_correspondences' records.
//   neighbour_snapshot_kernel        runs once per registration while the switch is on, behind the launch that produced the final
//                                    report: copies the status bytes and, per accepted point, the five neighbour indices of the last
//                                    k-NN sweep and the five map points they name -- the bits the last fit pass read
//   correspondence_geometry_kernel   the export: refits every accepted point from the snapshot with the fit pass's own code
//                                    (plane_fit.h), compacts the records in scan order, sums the labels' histogram in integers
// No registration kernel is changed and none takes part.
#include <hip/hip_runtime.h>

#include "plane_fit.h"  // (first: it defines and releases SO_UNROLL, which lm_solver.h -- behind corr_kernels.h -- defines for itself)

#include "corr_kernels.h"
#include "device_idioms.h"

namespace soicp {

// One thread per scan point.  Per point 1 status byte read and written; per accepted point 20 + 5 x 16 bytes read, 80 written.
__global__ __launch_bounds__(256) void neighbour_snapshot_kernel(const uint8_t* __restrict__ status, const uint32_t* __restrict__ nbr5,
                                                                 const float4* __restrict__ mpts, uint32_t n_map, uint32_t n,
                                                                 uint8_t* __restrict__ s_status, uint32_t* __restrict__ s_idx,
                                                                 float* __restrict__ s_pts) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint8_t st = status[i];
  s_status[i] = st;
  if (st != 0) return;  // MatchingResult::SUCCESS: the indices of any other point are stale
  uint32_t id[5];
#pragma unroll
  for (int t = 0; t < 5; ++t) id[t] = nbr5[(size_t)5 * i + t];
#pragma unroll
  for (int t = 0; t < 5; ++t) {
    const float4 p = id[t] < n_map ? mpts[id[t]] : make_float4(0.f, 0.f, 0.f, 0.f);
    s_idx[(size_t)5 * i + t] = id[t];
    s_pts[(size_t)15 * i + 3 * t] = p.x; s_pts[(size_t)15 * i + 3 * t + 1] = p.y; s_pts[(size_t)15 * i + 3 * t + 2] = p.z;
  }
}

void launch_neighbour_snapshot(const uint8_t* d_status, const uint32_t* d_nbr5, const float4* d_map_pts, uint32_t n_map, uint32_t n,
                               const NeighbourSnapshot& snap, hipStream_t s) {
  if (!n) return;
  neighbour_snapshot_kernel<<<(n + 255u) / 256u, 256, 0, s>>>(d_status, d_nbr5, d_map_pts, n_map, n, snap.status, snap.idx, snap.pts);
}

// One thread per scan point, tiles of kCorrTile consecutive points in ticket order, correspondences_kernel's order-preserving
// compaction (a ballot per round, the LDS prefix over (round, wavefront), lookback_exclusive, mbcnt; the count from the last tile) --
// but the ballots need the status bytes only, so the refit runs BEHIND the look-back, a round at a time, and nothing of a record
// stays in registers across it (a record is 48 words; correspondences_kernel's is 18 and is carried).
// Per accepted point: pw at pose_fit by the fit pass's own expression (kernels.hip eval_pass: quat_rotate in fp64, + t), the PCA,
// plane, gates and labels through plane_fit5_geometry with the fit pass's arguments, d2 through l2_d2 from the float query (float)pw.
// Every lane stores its own 192-byte record, 192 bytes from its neighbour's.  correspondences_kernel lays a round's 72-byte records out
// in LDS and stores consecutive words, measured there as the faster form; for this record the same form (48 KB of LDS) measured 30.0 /
// 30.5 / 30.3 us per launch on the 131 072-point scan against 28.5 / 28.1 / 27.9 us for the direct stores, alternating
// (profiles/correspondence_geometry/kernel_store_forms.txt), so the direct form is kept (the other: staged_store_not_kept.patch there).
// obs_hist: integer atomics in LDS, then one integer atomic per bin and tile -- the same sums in any order.
__global__ __launch_bounds__(256) void correspondence_geometry_kernel(const float* __restrict__ scan, const uint8_t* __restrict__ sstatus,
                                                                      const uint32_t* __restrict__ sidx, const float* __restrict__ spts, uint32_t n,
                                                                      Pose pose, float sq_max_dist_f, double max_point_dist,
                                                                      uint8_t* __restrict__ records, uint8_t* __restrict__ labels_out,
                                                                      double* __restrict__ refit_out, uint32_t* __restrict__ counts,
                                                                      int32_t* __restrict__ obs_hist, unsigned long long* __restrict__ state,
                                                                      uint32_t nblk) {
  constexpr int kPer = (int)(kCorrTile / 256u);
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  __shared__ unsigned long long s_bal[kPer * 4];  // (in LDS: the rounds behind the look-back are a loop, not unrolled)
  __shared__ int32_t s_hist[9];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(counts + 1, 1u);
  if (tid < 9) s_hist[tid] = 0;
  __syncthreads();
  const uint32_t bid = s_bid;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    const bool ok = i < n && sstatus[i] == 0;  // MatchingResult::SUCCESS
    const unsigned long long b = __ballot(ok);
    if (lane == 0) { s_bal[q * 4 + wave] = b; s_pre[q * 4 + wave] = (uint32_t)__popcll(b); }
  }
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in scan order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    const uint32_t excl = lookback_exclusive(state, bid, agg, lane);
    if (lane == 0) {
      if (bid == nblk - 1u) counts[0] = excl + agg;
      s_excl = excl;
    }
  }
  __syncthreads();
  const uint32_t excl = s_excl;
  const ObsAxes axes = obs_axes(pose);
#pragma unroll 1
  for (int q = 0; q < kPer; ++q) {
    const unsigned long long b = s_bal[q * 4 + wave];
    const bool mine = (b >> lane) & 1ull;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    const uint32_t first = s_pre[q * 4];
    uint32_t lab = 0x00FFFFFFu;  // 255 255 255: not an accepted point
    if (mine) {
      const uint32_t slot = s_pre[q * 4 + wave] - first + below;  // position among the round's accepted points
      uint32_t id[5];
      float nb[15];
#pragma unroll
      for (int t = 0; t < 5; ++t) id[t] = sidx[(size_t)5 * i + t];
#pragma unroll
      for (int t = 0; t < 15; ++t) nb[t] = spts[(size_t)15 * i + t];
      const double px = (double)scan[(size_t)i * 3], py = (double)scan[(size_t)i * 3 + 1], pz = (double)scan[(size_t)i * 3 + 2];
      double wx, wy, wz;
      quat_rotate<double>(pose.q, px, py, pz, wx, wy, wz);
      wx += pose.t[0]; wy += pose.t[1]; wz += pose.t[2];
      const double pw[3] = {wx, wy, wz};
      double nd[4] = {0, 0, 0, 0}, coeff = 0, ev[3] = {0, 0, 0}, nrm[3] = {0, 0, 0}, mean_abs = 0;
      int obs[3] = {255, 255, 255};
      const int fit = plane_fit5_geometry(nb, pw, axes, sq_max_dist_f, max_point_dist, nd, coeff, obs, ev, nrm, mean_abs);
      if (fit != SO_FIT_SUCCESS) {  // (never: the same code on the same bits accepted this point during the registration)
        atomicAdd(counts + 2, 1u);
        obs[0] = obs[1] = obs[2] = 255;
      } else {
        atomicAdd(&s_hist[obs[0]], 1); atomicAdd(&s_hist[obs[1]], 1); atomicAdd(&s_hist[obs[2]], 1);
      }
      lab = (uint32_t)obs[0] | ((uint32_t)obs[1] << 8) | ((uint32_t)obs[2] << 16);
      const float qx = (float)wx, qy = (float)wy, qz = (float)wz;
      // so_icp_correspondence_geometry_record: index nbr_index[5] | obs[3] reserved nbr[15] | d2[5] pad | pw | eig | pca_normal | mean_abs_dist
      uint32_t* o = reinterpret_cast<uint32_t*>(records + ((size_t)excl + first + slot) * kCorrGeomRecordBytes);
      double* od = reinterpret_cast<double*>(o);
      o[0] = i;
#pragma unroll
      for (int t = 0; t < 5; ++t) o[1 + t] = id[t];
      o[6] = lab;  // (reserved = 0)
#pragma unroll
      for (int t = 0; t < 15; ++t) o[7 + t] = __float_as_uint(nb[t]);
#pragma unroll
      for (int t = 0; t < 5; ++t) o[22 + t] = __float_as_uint(l2_d2(qx, qy, qz, nb[3 * t], nb[3 * t + 1], nb[3 * t + 2]));
      o[27] = 0u;
      od[14] = wx; od[15] = wy; od[16] = wz;
      od[17] = ev[0]; od[18] = ev[1]; od[19] = ev[2];
      od[20] = nrm[0]; od[21] = nrm[1]; od[22] = nrm[2];
      od[23] = mean_abs;
      if (refit_out) {  // so_icp_debug_correspondence_refit
        double* r = refit_out + (size_t)(excl + first + slot) * (kCorrRefitBytes / 8);
        r[0] = nd[0]; r[1] = nd[1]; r[2] = nd[2]; r[3] = nd[3]; r[4] = coeff;
      }
    }
    if (i < n) { labels_out[(size_t)3 * i] = (uint8_t)lab; labels_out[(size_t)3 * i + 1] = (uint8_t)(lab >> 8); labels_out[(size_t)3 * i + 2] = (uint8_t)(lab >> 16); }
  }
  __syncthreads();
  if (tid < 9 && s_hist[tid]) atomicAdd(&obs_hist[tid], s_hist[tid]);
}

void launch_correspondence_geometry(const CorrGeomIn& in, uint8_t* d_records, uint8_t* d_labels_out, double* d_refit_out, uint32_t* d_counts,
                                    int32_t* d_obs_hist, unsigned long long* d_state, hipStream_t s) {
  const uint32_t nblk = correspondence_workgroups(in.n);
  if (!nblk) return;
  correspondence_geometry_kernel<<<nblk, 256, 0, s>>>(in.scan, in.snap.status, in.snap.idx, in.snap.pts, in.n, in.pose_fit, in.sq_max_dist_f,
                                                      in.max_point_dist, d_records, d_labels_out, d_refit_out, d_counts, d_obs_hist, d_state, nblk);
}

}  // namespace soicp
