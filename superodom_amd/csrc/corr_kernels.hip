// corr_kernels.hip -- the export of a registration's plane correspondences (so_icp_correspondences): what the reference keeps in
// features_corres (LidarSlam.h:209-222, filled by extractFeaturesConstraints, LidarSlam.cpp:299-344) as one record per ACCEPTED scan
// point, in scan order, with the residual and the robust weight of the record at a pose of the caller's choice.
//   correspondences_kernel  reads the records the last fit pass left in memory (kernels.hip eval_pass: corr.nd / corr.coeff /
//                           corr.status, indexed like the scan) and the scan copy the registration kept; compacts the accepted ones
//   selection_correspondences_kernel  the same for a selection of kept sets, all in one launch: the hypotheses of
//                           so_icp_register_batch (so_icp_batch_correspondences) or the frames of a run, whose point counts differ
//                           (so_icp_sequence_correspondences); one text, two kernels: corr_export_body.inc
// Nothing here runs during a registration and no registration kernel is changed; residual, loss and weight are plane_factor.h's, as
// in eval_pass.
#include <hip/hip_runtime.h>

#include "corr_kernels.h"
#include "device_idioms.h"
#include "plane_factor.h"
#include "reg_plan.h"

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
#define SO_CORR_SELECTION 0
#include "corr_export_body.inc"
#undef SO_CORR_SELECTION
}

// so_icp_batch_correspondences / so_icp_sequence_correspondences: the same export for a SELECTION of kept sets in one launch.  Entry k is
// described by entries[k] (corr_kernels.h: where its records and its scan lie in the kept arrays, its point count -- 0 for an entry
// without a set --, its loss, its pose, where its records and its status row go); the entries have tile_first[k + 1] - tile_first[k]
// tiles each, possibly none.  A workgroup takes ONE global ticket and works on the entry and tile selection_ticket maps it to
// (reg_plan.h): it never depends on where the hardware placed it (blockIdx), only on workgroups that drew their tickets before it.
// Counts, tile costs and look-back words: counts[k], and the words tile_first[k] .. of tables of n_tiles words.
__global__ __launch_bounds__(256) void selection_correspondences_kernel(const float* __restrict__ scan_all, const double4* __restrict__ cnd_all,
                                                                        const double* __restrict__ ccoeff_all, const uint8_t* __restrict__ cstatus_all,
                                                                        const CorrSelEntry* __restrict__ entries, const uint32_t* __restrict__ tile_first,
                                                                        uint32_t n_sel, uint32_t n_tiles, uint8_t* __restrict__ records_all,
                                                                        uint8_t* __restrict__ status_all, uint32_t* __restrict__ counts,
                                                                        double* __restrict__ tile_cost_all, unsigned long long* __restrict__ state_all,
                                                                        uint32_t* __restrict__ ticket) {
#define SO_CORR_SELECTION 1
#include "corr_export_body.inc"
#undef SO_CORR_SELECTION
}

void launch_correspondences(const CorrExportIn& in, uint8_t* d_records, uint8_t* d_status_out, float* d_residual_out, uint32_t* d_n_accepted,
                            double* d_tile_cost, unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s) {
  const uint32_t nblk = correspondence_workgroups(in.n);
  if (!nblk) return;
  correspondences_kernel<<<nblk, 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.n, in.pose, in.a2, in.variant, d_records,
                                              d_status_out, d_residual_out, d_n_accepted, d_tile_cost, d_state, d_ticket, nblk);
}

void launch_selection_correspondences(const CorrSelIn& in, uint8_t* d_records, uint8_t* d_status_out, uint32_t* d_counts, double* d_tile_cost,
                                      unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s) {
  if (!in.n_tiles || !in.n_sel) return;
  selection_correspondences_kernel<<<in.n_tiles, 256, 0, s>>>(in.scan, in.corr.nd, in.corr.coeff, in.corr.status, in.entries, in.tile_first, in.n_sel,
                                                             in.n_tiles, d_records, d_status_out, d_counts, d_tile_cost, d_state, d_ticket);
}

}  // namespace soicp
