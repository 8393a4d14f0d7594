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

// ---- corr_sums_kernels.hip: so_icp_correspondence_sums, the sums of the kept set at poses of the caller's
// poses per call (the pose table's LDS), the sums of one pose (cost, count, Jtr[6], JtJ[21]: the head of LmSums), the words of an LmSums
constexpr uint32_t kCorrSumsMaxPoses = 64, kCorrSumsAcc = 29, kCorrSumsWords = 45;
static_assert(sizeof(LmSums) == kCorrSumsWords * sizeof(double) && offsetof(LmSums, hist) == kCorrSumsAcc * sizeof(double), "the kernels write LmSums records");
// what the kernels read of the set: CorrExportIn without a pose
struct CorrSumsIn {
  const float* scan;
  CorrBuffers corr;
  uint32_t n;
  double a2;
  int32_t variant;
};
struct CorrSumsHist { double v[16]; };  // LmSums::hist of every record written: the histograms the set was kept with
// d_poses: n_poses x 7 doubles (1 <= n_poses <= kCorrSumsMaxPoses); d_partials: n_poses x correspondence_workgroups(n) x kCorrSumsAcc
// doubles, every one written; d_sums_out: n_poses LmSums.  Two launches, nothing to clear.
void launch_correspondence_sums(const CorrSumsIn& in, const double* d_poses, uint32_t n_poses, const CorrSumsHist& hist, double* d_partials,
                                double* d_sums_out, hipStream_t s);

}  // namespace soicp
