// corr_sums_kernels.hip -- so_icp_correspondence_sums: cost and loss-corrected normal equations of the kept correspondence set
// (so_icp_keep_correspondences) at up to kCorrSumsMaxPoses poses of the caller's, summed on the device -- the per-LM-step evaluation of
// a host solver that takes its plane factors from so_icp_match / so_icp_correspondences.
//   correspondence_sums_kernel      reads what the export reads (the scan copy, corr.nd / corr.coeff / corr.status, in place), once per
//                                   point, and loops over the poses: one partial vector of the 29 sums per (tile, pose)
//   correspondence_sums_add_kernel  adds the tiles in tile order, one thread per (pose, component), into so_icp_sums records (a pose's
//                                   partial vectors reach its threads through LDS, 64 tiles at a time)
// Nothing here runs during a registration.  The per-point arithmetic is correspondences_kernel's (residual, loss: eval_pass's `at_pose`
// and `tail`, expression for expression) plus `tail`'s Jacobian row and sums; same headers, same -ffp-contract=off, the same explicit
// SO_FMA.  No atomics: every sum is a fixed tree, so two calls give the same bits, a pose's sums do not depend on the other poses of
// the call, and `cost` is so_icp_correspondences' cost at that pose bit for bit.
#include <hip/hip_runtime.h>

#include "corr_kernels.h"
#include "so_math.h"

namespace soicp {

namespace {
// a pose of the table in LDS: translation, quaternion, R(q) as Eigen::Quaternion::toRotationMatrix (eval_pass forms it the same way)
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
  __shared__ SumsPose s_pose[kCorrSumsMaxPoses];
  __shared__ double s_part[2][4][kAcc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t bid = blockIdx.x;
  if ((uint32_t)tid < n_poses) {
    SumsPose P;
    for (int k = 0; k < 3; ++k) P.t[k] = poses[(size_t)tid * 7 + k];
    for (int k = 0; k < 4; ++k) P.q[k] = poses[(size_t)tid * 7 + 3 + k];
    const double qx = P.q[0], qy = P.q[1], qz = P.q[2], qw = P.q[3];
    const double tx = 2 * qx, ty = 2 * qy, tz = 2 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx;
    const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    P.R[0] = 1 - (tyy + tzz); P.R[1] = txy - twz; P.R[2] = txz + twy;
    P.R[3] = txy + twz; P.R[4] = 1 - (txx + tzz); P.R[5] = tyz - twx;
    P.R[6] = txz - twy; P.R[7] = tyz + twx; P.R[8] = 1 - (txx + tyy);
    s_pose[tid] = P;
  }
  // (eval_pass: the quotient s / a^2 as a product with the reciprocal, the comparison on s itself)
  const double inv_a2 = 1.0 / a2, rho_out = (variant == 0) ? a2 / 6.0 : a2 / 3.0;
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
      const double px = pp[q][0], py = pp[q][1], pz = pp[q][2];
      double wx, wy, wz;
      quat_rotate<double>(P.q, px, py, pz, wx, wy, wz);  // at_pose
      wx += P.t[0]; wy += P.t[1]; wz += P.t[2];
      const double r = SO_FMA(nd[q].x, wx, SO_FMA(nd[q].y, wy, SO_FMA(nd[q].z, wz, nd[q].w)));  // tail
      const double s = r * r;
      double rho0, rho1;
      if (s <= a2) {
        const double v = 1.0 - s * inv_a2, v2 = v * v;
        rho0 = rho_out * (1.0 - v2 * v); rho1 = (variant == 0) ? 0.5 * v2 : v2;
      } else {
        rho0 = rho_out; rho1 = 0;
      }
      const double w = co[q] * rho1;
      // J = [n^T, (p x R^T n)^T]  (lidarOptimization.cpp:68-74)
      const double m0 = SO_FMA(P.R[0], nd[q].x, SO_FMA(P.R[3], nd[q].y, P.R[6] * nd[q].z));
      const double m1 = SO_FMA(P.R[1], nd[q].x, SO_FMA(P.R[4], nd[q].y, P.R[7] * nd[q].z));
      const double m2 = SO_FMA(P.R[2], nd[q].x, SO_FMA(P.R[5], nd[q].y, P.R[8] * nd[q].z));
      const double J[6] = {nd[q].x, nd[q].y, nd[q].z, SO_FMA(py, m2, -(pz * m1)), SO_FMA(pz, m0, -(px * m2)), SO_FMA(px, m1, -(py * m0))};
      acc[0] = SO_FMA(0.5 * co[q], rho0, acc[0]);
      acc[1] += 1.0;
      const double wr = w * r;
      int e = 8;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        acc[2 + a] = SO_FMA(J[a], wr, acc[2 + a]);
        const double wj = w * J[a];
#pragma unroll
        for (int b = a; b < 6; ++b) { acc[e] = SO_FMA(wj, J[b], acc[e]); ++e; }
      }
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
