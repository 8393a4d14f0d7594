// corr_kernels.hip -- the export of a registration's plane correspondences (so_icp_correspondences): what the reference keeps in
// features_corres (LidarSlam.h:209-222, filled by extractFeaturesConstraints, LidarSlam.cpp:299-344) as one record per ACCEPTED scan
// point, in scan order, with the residual and the robust weight of the record at a pose of the caller's choice.
//   correspondences_kernel  reads the records the last fit pass left in memory (kernels.hip eval_pass: corr.nd / corr.coeff /
//                           corr.status, indexed like the scan) and the scan copy the registration kept; compacts the accepted ones
// Nothing here runs during a registration and no registration kernel is changed; residual, loss and weight are plane_factor.h's, as
// in eval_pass.
#include <hip/hip_runtime.h>

#include "corr_kernels.h"
#include "device_idioms.h"
#include "plane_factor.h"

namespace soicp {

// One thread per scan point, tiles of kCorrTile consecutive points in ticket order, registered_scan_kernel's order-preserving
// compaction: a ballot per round, the LDS prefix over (round, wavefront), lookback_exclusive, mbcnt; the count from the last tile.
// Per point: 1 status byte read, 1 status byte + 1 float written; per accepted point 32 + 8 + 12 bytes read and one 72-byte record
// written, a round's records through LDS so that the workgroup stores consecutive 8-byte words.
// The cost of the set, sum 0.5 c rho(r^2), is a fixed tree: a thread adds its rounds in round order, a wavefront its lanes by
// butterfly, the tile its four wavefronts in wavefront order; the host adds the tiles in tile order -- the same bits on every call.
__global__ __launch_bounds__(256) void correspondences_kernel(const float* __restrict__ scan, const double4* __restrict__ cnd,
                                                              const double* __restrict__ ccoeff, const uint8_t* __restrict__ cstatus, uint32_t n,
                                                              Pose pose, double a2, int variant, uint8_t* __restrict__ records,
                                                              uint8_t* __restrict__ status_out, float* __restrict__ residual_out,
                                                              uint32_t* __restrict__ n_accepted, double* __restrict__ tile_cost,
                                                              unsigned long long* __restrict__ state, uint32_t* __restrict__ ticket, uint32_t nblk) {
  constexpr int kPer = (int)(kCorrTile / 256u);
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  __shared__ double s_cost[4];
  __shared__ uint2 s_rec[256 * (kCorrRecordBytes / 8)];  // the records of one round, in output order
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const TukeyLoss L(a2, variant);
  unsigned long long bal[kPer];
  float pf[kPer][3];
  double4 nd[kPer];
  double co[kPer], res[kPer], wgt[kPer];
  double cost = 0;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    bool ok = false;
    pf[q][0] = pf[q][1] = pf[q][2] = 0.0f;
    nd[q] = make_double4(0, 0, 0, 0); co[q] = 0; res[q] = 0; wgt[q] = 0;
    if (i < n) {
      const uint8_t status = cstatus[i];
      ok = status == 0;  // MatchingResult::SUCCESS
      float rf = __builtin_nanf("");
      if (ok) {
        pf[q][0] = scan[(size_t)i * 3]; pf[q][1] = scan[(size_t)i * 3 + 1]; pf[q][2] = scan[(size_t)i * 3 + 2];
        nd[q] = cnd[i]; co[q] = ccoeff[i];
        const double r = plane_residual_at(pose.q, pose.t, (double)pf[q][0], (double)pf[q][1], (double)pf[q][2], nd[q].x, nd[q].y, nd[q].z, nd[q].w);
        double rho0, rho1;
        tukey_rho(L, r * r, rho0, rho1);
        res[q] = r; wgt[q] = co[q] * rho1;
        cost = SO_FMA(0.5 * co[q], rho0, cost);
        rf = (float)r;
      }
      status_out[i] = status;
      residual_out[i] = rf;
    }
    bal[q] = __ballot(ok);
    if (lane == 0) s_pre[q * 4 + wave] = (uint32_t)__popcll(bal[q]);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) cost += __shfl_xor(cost, d, 64);
  if (lane == 0) s_cost[wave] = cost;
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in scan order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
    tile_cost[bid] = ((s_cost[0] + s_cost[1]) + s_cost[2]) + s_cost[3];
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    const uint32_t excl = lookback_exclusive(state, bid, agg, lane);
    if (lane == 0) {
      if (bid == nblk - 1u) *n_accepted = excl + agg;
      s_excl = excl;
    }
  }
  __syncthreads();
  const uint32_t excl = s_excl;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const bool mine = (bal[q] >> lane) & 1ull;
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[q], 0u));
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    // The round's records are one contiguous range of the output: laid out in LDS, then stored by the whole workgroup, lane after
    // lane (a lane storing its own 72-byte record, 72 bytes from its neighbour's, measured 0.3 - 1.4 us slower per 131 072-point scan)
    const uint32_t first = s_pre[q * 4], count = (q + 1 < kPer ? s_pre[(q + 1) * 4] : s_agg) - first;
    if (mine) {  // so_icp_correspondence: index, p[3] | n[3] | d | coeff | residual | weight
      uint2* o = s_rec + (size_t)(s_pre[q * 4 + wave] - first + below) * (kCorrRecordBytes / 8);
      double* od = reinterpret_cast<double*>(o);
      o[0] = make_uint2(i, __float_as_uint(pf[q][0]));
      o[1] = make_uint2(__float_as_uint(pf[q][1]), __float_as_uint(pf[q][2]));
      od[2] = nd[q].x; od[3] = nd[q].y; od[4] = nd[q].z; od[5] = nd[q].w;
      od[6] = co[q]; od[7] = res[q]; od[8] = wgt[q];
    }
    __syncthreads();
    uint2* out8 = reinterpret_cast<uint2*>(records + ((size_t)excl + first) * kCorrRecordBytes);
    for (uint32_t w = (uint32_t)tid; w < count * (kCorrRecordBytes / 8); w += 256u) out8[w] = s_rec[w];
    __syncthreads();
  }
}

void launch_correspondences(const CorrExportIn& in, uint8_t* d_records, uint8_t* d_status_out, float* d_residual_out, uint32_t* d_n_accepted,
                            double* d_tile_cost, unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s) {
  const uint32_t nblk = correspondence_workgroups(in.n);
  if (!nblk) return;
  correspondences_kernel<<<nblk, 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.n, in.pose, in.a2, in.variant, d_records,
                                              d_status_out, d_residual_out, d_n_accepted, d_tile_cost, d_state, d_ticket, nblk);
}

}  // namespace soicp
