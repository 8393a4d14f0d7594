// corr_kernels.h -- launcher of corr_kernels.hip: the export of the last registration's plane correspondences
// (so_icp_correspondences; the reference's features_corres, LidarSlam.h:209-222).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "kernels.h"

namespace soicp {

// points per workgroup of the export's compaction (4 rounds of 256), bytes of one so_icp_correspondence
constexpr uint32_t kCorrTile = 1024;
constexpr uint32_t kCorrRecordBytes = 72;
inline uint32_t correspondence_workgroups(uint32_t n) { return (n + kCorrTile - 1u) / kCorrTile; }

// What the export reads: the packed scan the registration kept, the records its last fit pass stored (CorrBuffers, indexed like the
// scan), the evaluation pose and the loss of THAT registration (EvalParams::a2 / ::variant)
struct CorrExportIn {
  const float* scan;
  CorrBuffers corr;
  uint32_t n;
  Pose pose;
  double a2;
  int32_t variant;
};
// d_records: room for n records of kCorrRecordBytes (8-byte aligned); d_status_out n bytes; d_residual_out n floats; d_tile_cost and
// d_state correspondence_workgroups(n) words each.  d_state, d_ticket and *d_n_accepted zeroed by the caller.
void launch_correspondences(const CorrExportIn& in, uint8_t* d_records, uint8_t* d_status_out, float* d_residual_out, uint32_t* d_n_accepted,
                            double* d_tile_cost, unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s);

}  // namespace soicp
