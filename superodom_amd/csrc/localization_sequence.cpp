// localization_sequence.cpp -- so_icp_localization_sequence: a run of frames in the reference's per-frame order.
//
// LidarSLAM::Localization (LidarSlam.cpp:30-51) registers a frame and always inserts it (performPostOptimizationProcessing ->
// transformAndAddToMap, LidarSlam.cpp:154-167; checkMotionThresholds returns true, :193), and the node chains the next guess from the
// pose Localization returned (laserMapping.cpp:345-372: T_w_lidar = T_w_lidar * prediction).  This entry runs that loop over a
// recorded run (a log replayed, a map built offline): for every frame exactly the so_icp_localization(_dev) call a caller's own loop
// would make, so poses, statistics and the map after every frame are the per-frame loop's by construction.
//
// A convenience entry, not a faster path: the frames run one after the other through the per-frame entry points, the guesses composed
// on the host (pose_compose, the arithmetic the node's `T_w_lidar * prediction` reduces to).  Registration k + 1 is not enqueued before
// the host has read frame k's report -- the insert of frame k needs pose_out_k, which the host computes (MannualYawCorrection in host
// libm, fill_result) -- so the device idles between an insert and the next registration as it does in a caller's own loop
// (profiles/localization_sequence/).
#include <cstring>
#include <string>

#include "ctx.h"

extern "C" {

int so_icp_localization_sequence(so_icp_ctx* c, int count, const void* const* scans, const size_t* n_points, size_t stride_bytes,
                                 int scans_on_device, const double pose0[7], const double* deltas, const double* times, double* poses_out,
                                 double* guesses_out, so_icp_stats* stats, int* n_done) {
  if (n_done) *n_done = 0;
  if (!c || count < 0 || (count && (!scans || !n_points || !pose0 || !times || !poses_out)) || (count > 1 && !deltas)) return SO_ICP_E_INVALID;
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4 || stride_bytes < 12) return fail(c, SO_ICP_E_INVALID, "so_icp_localization_sequence: stride_bytes must be a multiple of 4, >= 12");
  if (scans_on_device && stride_bytes != 12) return fail(c, SO_ICP_E_INVALID, "so_icp_localization_sequence: resident scans are packed xyz (stride 12)");
  for (int k = 0; k < count; ++k)
    if (!scans[k] && n_points[k]) return fail(c, SO_ICP_E_INVALID, "so_icp_localization_sequence: scans[" + std::to_string(k) + "] is NULL");
  if (count == 0) return SO_ICP_OK;
  NEED_DEVICE(c);
  if (const int rc = refuse_pending(c, "so_icp_localization_sequence", kPriorsRun)) return rc;
  // so_icp_set_sequence_priors: one prior per frame of this call (another length: refused, they stay pending); taken out of the context
  // here -- consumed whatever this call returns --, frame k's goes in as the single prior its per-frame entry consumes
  if (!c->pending.count_matches(kPriorsRun, count)) return fail(c, SO_ICP_E_INVALID, "so_icp_localization_sequence: count differs from that of the pending so_icp_set_sequence_priors call");
  // so_icp_keep_sequence_correspondences: the set of this run, reserved before its first launch; every frame's registration copies its
  // scan and the context's records into its slice behind its report and in front of its insert (seq_corr_note_plain).  Before the
  // priors are taken: SO_ICP_E_NOMEM leaves them pending
  bool keep = false;
  if (keeps_sequence_correspondences(c)) {
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    if (const int rc = seq_corr_begin(c, count, n_points)) return rc;
    keep = c->seq_corr->valid;
  }
  const PriorSet run_priors = c->pending.take(kPriorsRun);
  struct Frame { so_icp_ctx* c; ~Frame() { c->seq_corr_frame = -1; } } frame{c};

  double guess[7];
  std::memcpy(guess, pose0, sizeof(guess));
  for (int k = 0; k < count; ++k) {
    // guess_k = pose_out_(k-1) o delta_k: the pose Localization returned, after MannualYawCorrection (LidarSlam.cpp:891-913) --
    // so_icp_register_sequence chains from the optimised pose before that correction instead
    if (k) pose_compose(poses_out + 7 * (size_t)(k - 1), deltas + 7 * (size_t)k, guess);
    if (guesses_out) std::memcpy(guesses_out + 7 * (size_t)k, guess, sizeof(guess));
    double* pose_out = poses_out + 7 * (size_t)k;
    so_icp_stats local;
    so_icp_stats* st = stats ? stats + k : &local;
    run_priors.arm(c, k, guess);
    c->seq_corr_frame = keep ? k : -1;
    const int rc = scans_on_device
                       ? so_icp_localization_dev(c, 1, guess, scans[k], n_points[k], times[k], pose_out, st)
                       : so_icp_localization(c, 1, guess, static_cast<const float*>(scans[k]), n_points[k], stride_bytes, times[k], pose_out, st);
    if (rc < 0 && keep) seq_corr_fail(c);  // (a run that failed leaves no frame's set)
    if (rc != SO_ICP_OK) return rc;  // SO_ICP_NOT_ENOUGH_MAP_FEATURES or an error: the run stops at this frame (neither accepted nor inserted)
    if (n_done) *n_done = k + 1;
  }
  return SO_ICP_OK;
}

}  // extern "C"
