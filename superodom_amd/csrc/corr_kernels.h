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

// ---- the exports over a SELECTION of kept sets -- so_icp_batch_correspondences / so_icp_batch_correspondence_sums (the hypotheses of
// so_icp_register_batch) and so_icp_sequence_correspondences / so_icp_sequence_correspondence_sums (the frames of a run): one launch of
// selection_correspondences_kernel (corr_kernels.hip), two of selection_correspondence_sums_kernel and its add kernel
// (corr_sums_kernels.hip), whichever of the two the selection comes from.
// One entry of the selection, as the kernels read it from a device table: where the entry's records lie in the kept arrays (element
// `at` of nd / coeff / status) and where its scan lies (point `scan_at` of the packed scans: a run keeps a scan per frame beside its
// records, a batch one scan for all hypotheses), where its records and its status row go, the loss of THAT registration, the
// evaluation pose (the export; the sums have a pose table of their own) and its points (0: an entry without a set, or an empty scan)
struct CorrSelEntry {
  unsigned long long at, rec_first, status_first;
  double a2;
  double pose[7];
  uint32_t n;
  int32_t variant;
  unsigned long long scan_at;
};
static_assert(sizeof(CorrSelEntry) == 104 && offsetof(CorrSelEntry, scan_at) == 96, "the host fills a table of these");
// What they read: the packed scans and the records of ALL entries of the kept set, the entry table and the prefix table of the entries'
// tile counts (n_sel + 1 words, reg_plan.h: selection_tile_table), both on the device; n_tiles = tile_first[n_sel], max_tiles the tiles
// of the largest entry
struct CorrSelIn {
  const float* scan;
  CorrBuffers corr;
  const CorrSelEntry* entries;
  const uint32_t* tile_first;
  uint32_t n_sel, n_tiles, max_tiles;
};
// d_records: room for the last entry's offset + the points of the largest selected entry; d_status_out: the rows of all entries;
// d_counts n_sel words; d_tile_cost and d_state n_tiles words each.  d_state, d_ticket and d_counts zeroed by the caller.  One launch of
// n_tiles workgroups.
void launch_selection_correspondences(const CorrSelIn& in, uint8_t* d_records, uint8_t* d_status_out, uint32_t* d_counts, double* d_tile_cost,
                                      unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s);
// d_poses: n_sel x n_poses x 7 doubles; d_hists: n_sel x 16 doubles; d_partials: n_tiles x n_poses x kCorrSumsAcc doubles (entry e at
// tile_first[e] x n_poses vectors, [pose][tile] inside), every one written; d_sums_out: n_sel x n_poses LmSums.  Two launches, the first
// of max_tiles x n_sel workgroups.
void launch_selection_correspondence_sums(const CorrSelIn& in, const double* d_poses, uint32_t n_poses, const double* d_hists, double* d_partials,
                                          double* d_sums_out, hipStream_t s);

// ---- corr_geometry_kernels.hip: so_icp_correspondence_geometry, the neighbours, PCA and observability labels of the kept set
// bytes of one so_icp_correspondence_geometry_record; the refit's plane of so_icp_debug_correspondence_refit (n[3], d, coeff)
constexpr uint32_t kCorrGeomRecordBytes = 192, kCorrRefitBytes = 40;
// The snapshot a registration leaves while the switch is on, indexed like the scan: the status bytes, and for a point of status 0 its
// five neighbour indices and the five map points they name
struct NeighbourSnapshot {
  uint8_t* status;   // n
  uint32_t* idx;     // 5 n
  float* pts;        // 15 n
};
// One launch: copies status[i], and where it is 0, nbr5[5 i ..] and map_pts[those].  n_map: the extent of map_pts in points (of the
// device map's pool: its slots x kCapPerSlot); an index beyond it, which no accepted point holds, would be left as zeros
void launch_neighbour_snapshot(const uint8_t* d_status, const uint32_t* d_nbr5, const float4* d_map_pts, uint32_t n_map, uint32_t n,
                               const NeighbourSnapshot& snap, hipStream_t s);
// What the export reads: the packed scan the registration kept, the snapshot, the pose the set was formed at and the gates of THAT
// registration (MatchParams::sq_max_dist_f / ::max_point_dist)
struct CorrGeomIn {
  const float* scan;
  NeighbourSnapshot snap;
  uint32_t n;
  Pose pose_fit;
  float sq_max_dist_f;
  double max_point_dist;
};
// d_records: room for n records of kCorrGeomRecordBytes (8-byte aligned); d_labels_out 3 n bytes; d_refit_out nullable, n x
// kCorrRefitBytes; d_counts {n_accepted, ticket, points whose refit was not accepted, -} and d_obs_hist 9 int32, d_state
// correspondence_workgroups(n) words: all zeroed by the caller.
void launch_correspondence_geometry(const CorrGeomIn& in, uint8_t* d_records, uint8_t* d_labels_out, double* d_refit_out, uint32_t* d_counts,
                                    int32_t* d_obs_hist, unsigned long long* d_state, hipStream_t s);

}  // namespace soicp
