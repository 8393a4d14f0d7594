// corr_sums_kernels.hip -- so_icp_correspondence_sums: cost and loss-corrected normal equations of the kept correspondence set
// (so_icp_keep_correspondences) at up to kCorrSumsMaxPoses poses of the caller's, summed on the device -- the per-LM-step evaluation of
// a host solver that takes its plane factors from so_icp_match / so_icp_correspondences.
//   correspondence_sums_kernel      reads what the export reads (the scan copy, corr.nd / corr.coeff / corr.status, in place), once per
//                                   point, and loops over the poses: one partial vector of the 29 sums per (tile, pose)
//   correspondence_sums_add_kernel  adds the tiles in tile order, one thread per (pose, component), into so_icp_sums records (a pose's
//                                   partial vectors reach its threads through LDS, 64 tiles at a time)
// Nothing here runs during a registration.  The per-point arithmetic is plane_factor.h's, as in eval_pass and correspondences_kernel.
// No atomics: every sum is a fixed tree, so two calls give the same bits, a pose's sums do not depend on the other poses of the call,
// and `cost` is so_icp_correspondences' cost at that pose bit for bit.
#include <hip/hip_runtime.h>

#include "corr_kernels.h"
#include "plane_factor.h"

namespace soicp {

namespace {
// a pose of the table in LDS: translation, quaternion, R(q) (quat_to_matrix)
struct SumsPose { double t[3], q[4], R[9]; };
}  // namespace

// The export's launch shape: one thread per point, workgroups of 256, tiles of kCorrTile consecutive points (tile = workgroup index:
// nothing is compacted, so no ticket).  A thread loads its kCorrTile / 256 points once, then per pose: its rounds in round order, a
// butterfly over the wavefront, the four wavefronts in wavefront order -- correspondences_kernel's tree for its cost, here for all 29
// sums (cost, count, Jtr[6], JtJ[21]).  partials: [pose][tile][kCorrSumsAcc].
__global__ __launch_bounds__(256) void correspondence_sums_kernel(const float* __restrict__ scan, const double4* __restrict__ cnd,
                                                                  const double* __restrict__ ccoeff, const uint8_t* __restrict__ cstatus, uint32_t n,
                                                                  const double* __restrict__ poses, uint32_t n_poses, double a2, int variant,
                                                                  double* __restrict__ partials) {
  constexpr int kPer = (int)(kCorrTile / 256u), kAcc = (int)kCorrSumsAcc;
  static_assert(kAcc == kPlaneFactorSums, "plane_factor_add fills a partial vector");
  __shared__ SumsPose s_pose[kCorrSumsMaxPoses];
  __shared__ double s_part[2][4][kAcc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t bid = blockIdx.x;
  if ((uint32_t)tid < n_poses) {
    SumsPose P;
    for (int k = 0; k < 3; ++k) P.t[k] = poses[(size_t)tid * 7 + k];
    for (int k = 0; k < 4; ++k) P.q[k] = poses[(size_t)tid * 7 + 3 + k];
    quat_to_matrix(P.q, P.R);
    s_pose[tid] = P;
  }
  const TukeyLoss L(a2, variant);
  bool ok[kPer];
  double pp[kPer][3];
  double4 nd[kPer];
  double co[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kCorrTile + (uint32_t)q * 256u + (uint32_t)tid;
    ok[q] = false;
    pp[q][0] = pp[q][1] = pp[q][2] = 0;
    nd[q] = make_double4(0, 0, 0, 0); co[q] = 0;
    if (i < n && cstatus[i] == 0) {  // MatchingResult::SUCCESS
      ok[q] = true;
      pp[q][0] = (double)scan[(size_t)i * 3]; pp[q][1] = (double)scan[(size_t)i * 3 + 1]; pp[q][2] = (double)scan[(size_t)i * 3 + 2];
      nd[q] = cnd[i]; co[q] = ccoeff[i];
    }
  }
  __syncthreads();
  for (uint32_t k = 0; k < n_poses; ++k) {
    const SumsPose& P = s_pose[k];
    double acc[kAcc];
#pragma unroll
    for (int a = 0; a < kAcc; ++a) acc[a] = 0;
#pragma unroll
    for (int q = 0; q < kPer; ++q) {
      if (!ok[q]) continue;
      const double r = plane_residual_at(P.q, P.t, pp[q][0], pp[q][1], pp[q][2], nd[q].x, nd[q].y, nd[q].z, nd[q].w);
      double rho0, rho1;
      tukey_rho(L, r * r, rho0, rho1);
      plane_factor_add(P.R, pp[q][0], pp[q][1], pp[q][2], nd[q].x, nd[q].y, nd[q].z, co[q], r, rho0, co[q] * rho1, acc);
    }
#pragma unroll
    for (int a = 0; a < kAcc; ++a) {
      double v = acc[a];
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
      acc[a] = v;
    }
    // (two buffers: the readers of pose k are past the barrier of pose k + 1 before pose k + 2 is written)
    double (*part)[kAcc] = s_part[k & 1u];
    if (lane == 0) {
#pragma unroll
      for (int a = 0; a < kAcc; ++a) part[wave][a] = acc[a];
    }
    __syncthreads();
    if (tid < kAcc) partials[((size_t)k * gridDim.x + bid) * kAcc + tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
  }
}

// One workgroup per pose, one thread per word of its so_icp_sums: the 29 sums as the tiles' partial sums added in tile order from +0.0
// (the order in which so_icp_correspondences adds its tile costs on the host), then the 16 histogram words the set was kept with.
// A thread that fetched its 128 partials one after the other from memory spent 30 us of a 57 us call on the load latencies (measured,
// profiles/seam_c/README.md): the pose's partial vectors are contiguous, so the whole workgroup brings kChunk tiles of them into LDS
// with consecutive loads, and threads 0 .. 28 add them from there -- the same additions in the same order.
__global__ __launch_bounds__(256) void correspondence_sums_add_kernel(const double* __restrict__ partials, uint32_t nblk, CorrSumsHist hist,
                                                                      double* __restrict__ sums_out) {
  constexpr uint32_t kAcc = kCorrSumsAcc, kWords = kCorrSumsWords, kChunk = 64;
  __shared__ double s_in[kChunk * kAcc];
  const uint32_t k = blockIdx.x, tid = threadIdx.x;
  const double* mine = partials + (size_t)k * nblk * kAcc;
  double v = 0;
  for (uint32_t b0 = 0; b0 < nblk; b0 += kChunk) {
    const uint32_t tiles = nblk - b0 < kChunk ? nblk - b0 : kChunk;
    for (uint32_t w = tid; w < tiles * kAcc; w += 256u) s_in[w] = mine[(size_t)b0 * kAcc + w];
    __syncthreads();
    if (tid < kAcc)
      for (uint32_t b = 0; b < tiles; ++b) v += s_in[b * kAcc + tid];
    __syncthreads();
  }
  if (tid < kAcc) sums_out[(size_t)k * kWords + tid] = v;
  else if (tid < kWords) sums_out[(size_t)k * kWords + tid] = hist.v[tid - kAcc];
}

void launch_correspondence_sums(const CorrSumsIn& in, const double* d_poses, uint32_t n_poses, const CorrSumsHist& hist, double* d_partials,
                                double* d_sums_out, hipStream_t s) {
  const uint32_t nblk = correspondence_workgroups(in.n);
  if (!n_poses || n_poses > kCorrSumsMaxPoses) return;
  if (nblk)
    correspondence_sums_kernel<<<nblk, 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.n, d_poses, n_poses, in.a2, in.variant, d_partials);
  correspondence_sums_add_kernel<<<n_poses, 256, 0, s>>>(d_partials, nblk, hist, d_sums_out);
}

}  // namespace soicp
