// corr_sums_kernels.hip -- so_icp_correspondence_sums: cost and loss-corrected normal equations of the kept correspondence set
// (so_icp_keep_correspondences) at up to kCorrSumsMaxPoses poses of the caller's, summed on the device -- the per-LM-step evaluation of
// a host solver that takes its plane factors from so_icp_match / so_icp_correspondences.
//   correspondence_sums_kernel      reads what the export reads (the scan copy, corr.nd / corr.coeff / corr.status, in place), once per
//                                   point, and loops over the poses: one partial vector of the 29 sums per (tile, pose)
//   correspondence_sums_add_kernel  adds the tiles in tile order, one thread per (pose, component), into so_icp_sums records (a pose's
//                                   partial vectors reach its threads through LDS, 64 tiles at a time)
//   selection_correspondence_sums_kernel, selection_correspondence_sums_add_kernel  the same two for a selection of kept sets in one
//                                   launch each: the hypotheses of so_icp_register_batch (so_icp_batch_correspondence_sums) or the
//                                   frames of a run, whose point counts differ (so_icp_sequence_correspondence_sums); one text per
//                                   pair, two kernels each: corr_sums_body.inc
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
#define SO_SUMS_ADD 0
#define SO_SUMS_SELECTION 0
#include "corr_sums_body.inc"
#undef SO_SUMS_SELECTION
#undef SO_SUMS_ADD
}
// so_icp_batch_correspondence_sums / so_icp_sequence_correspondence_sums: grid (tiles of the largest entry, entries of the selection).
// Workgroup (b, k) is tile b of entry k, and leaves at once where the entry has fewer tiles (nothing is compacted, so the launch index
// serves and no ticket is drawn).  An entry's records, scan and loss come from entries[entry], its n_poses poses -- the table in LDS --
// from poses_all[entry][..][7]; its partial vectors lie at tile_first[entry] x n_poses of partials_all, [pose][tile] inside.
__global__ __launch_bounds__(256) void selection_correspondence_sums_kernel(const float* __restrict__ scan_all, const double4* __restrict__ cnd_all,
                                                                            const double* __restrict__ ccoeff_all, const uint8_t* __restrict__ cstatus_all,
                                                                            const CorrSelEntry* __restrict__ entries, const uint32_t* __restrict__ tile_first,
                                                                            const double* __restrict__ poses_all, uint32_t n_poses,
                                                                            double* __restrict__ partials_all) {
#define SO_SUMS_ADD 0
#define SO_SUMS_SELECTION 1
#include "corr_sums_body.inc"
#undef SO_SUMS_SELECTION
#undef SO_SUMS_ADD
}

// One workgroup per pose, one thread per word of its so_icp_sums: the 29 sums as the tiles' partial sums added in tile order from +0.0
// (the order in which so_icp_correspondences adds its tile costs on the host), then the 16 histogram words the set was kept with.
// A thread that fetched its 128 partials one after the other from memory spent 30 us of a 57 us call on the load latencies (measured,
// profiles/seam_c/README.md): the pose's partial vectors are contiguous, so the whole workgroup brings kChunk tiles of them into LDS
// with consecutive loads, and threads 0 .. 28 add them from there -- the same additions in the same order.
__global__ __launch_bounds__(256) void correspondence_sums_add_kernel(const double* __restrict__ partials, uint32_t nblk, CorrSumsHist hist,
                                                                      double* __restrict__ sums_out) {
#define SO_SUMS_ADD 1
#define SO_SUMS_SELECTION 0
#include "corr_sums_body.inc"
#undef SO_SUMS_SELECTION
#undef SO_SUMS_ADD
}

// One workgroup per (entry, pose) of the selection: the entry's own number of tiles, added in tile order (none: +0.0 throughout), then
// the 16 histogram words of the entry's hypothesis or frame (hists: [entry][16])
__global__ __launch_bounds__(256) void selection_correspondence_sums_add_kernel(const double* __restrict__ partials, const uint32_t* __restrict__ tile_first,
                                                                                uint32_t n_poses, const double* __restrict__ hists,
                                                                                double* __restrict__ sums_out) {
#define SO_SUMS_ADD 1
#define SO_SUMS_SELECTION 1
#include "corr_sums_body.inc"
#undef SO_SUMS_SELECTION
#undef SO_SUMS_ADD
}

void launch_correspondence_sums(const CorrSumsIn& in, const double* d_poses, uint32_t n_poses, const CorrSumsHist& hist, double* d_partials,
                                double* d_sums_out, hipStream_t s) {
  const uint32_t nblk = correspondence_workgroups(in.n);
  if (!n_poses || n_poses > kCorrSumsMaxPoses) return;
  if (nblk)
    correspondence_sums_kernel<<<nblk, 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.n, d_poses, n_poses, in.a2, in.variant, d_partials);
  correspondence_sums_add_kernel<<<n_poses, 256, 0, s>>>(d_partials, nblk, hist, d_sums_out);
}

void launch_selection_correspondence_sums(const CorrSelIn& in, const double* d_poses, uint32_t n_poses, const double* d_hists, double* d_partials,
                                          double* d_sums_out, hipStream_t s) {
  if (!in.n_sel || !n_poses || n_poses > kCorrSumsMaxPoses) return;
  if (in.n_tiles)
    selection_correspondence_sums_kernel<<<dim3(in.max_tiles, in.n_sel), 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.entries,
                                                                                     in.tile_first, d_poses, n_poses, d_partials);
  selection_correspondence_sums_add_kernel<<<in.n_sel * n_poses, 256, 0, s>>>(d_partials, in.tile_first, n_poses, d_hists, d_sums_out);
}

}  // namespace soicp
