// batch.cpp -- so_icp_register_batch: B hypotheses of one scan in the same launches.
//
// One binning launch sequence over (queries x hypotheses), then rounds of { one k-NN launch over the chunks of every
// hypothesis still iterating, one persistent solve launch in which every such hypothesis owns a group of workgroups
// and runs its own LM controller (kernels.hip: solve_kernel<BATCH>) , one read-back of the state blocks }.  A hypothesis
// is an independent registration: it leaves the rounds when its own termination rule fires (LidarSlam.cpp:141), and the
// workgroups it held go to the others in the next round.  Results are bit-identical to so_icp_register per hypothesis.
// so_icp_set_batch_priors: every hypothesis may carry a pose prior of its own -- a table of prior blocks copied in front of round 0,
// read by solve_kernel_batch_prior, which a round launches only where a hypothesis of its list carries one (reg_plan.h).
// so_icp_keep_batch_correspondences: while the switch is on, a group's kernels write their records into the slices of the kept set
// (other kernel arguments, the same kernels) and a lane copies its context's records there; selection_correspondences.cpp exports them.
// so_icp_match_batch: the same scan MATCHED at many poses, nothing solved -- a group's set-up and round 0's sweep, then ONE launch that fits
// and evaluates every (pose, point) (kernels.hip: match_batch_kernel); no workgroup of it waits for another, so none of the residency
// rules below apply to it.  It leaves the batch's kept set like a batch does.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"

namespace {

constexpr int kBatchMaxConcurrent = 64;
// element stride of a hypothesis' arrays for a scan of n points
uint32_t batch_stride(size_t n) { return (uint32_t)(((n + 256 + 63) / 64) * 64); }
int batch_reserve(so_icp_ctx* c, uint32_t B, size_t n, uint32_t lg) {
  so_icp_ctx::BatchBufs& b = c->batch;
  const uint32_t bs = batch_stride(n);
  const size_t T = (size_t)1 << lg;
  const size_t partial_bytes = (size_t)kFitBlocksMax * kRecordChunksMax * 16;
  if (B > b.cap_hyp || bs > b.bs || lg != b.table_log2) {
    const uint32_t cap = std::max(B, b.cap_hyp), nbs = std::max(bs, b.bs);
    b.release();
    HIP_TRY(c, b.states.reserve((size_t)cap * sizeof(DevState))); HIP_TRY(c, b.begin.reserve((size_t)cap * sizeof(RegBeginArgs)));
    HIP_TRY(c, b.active.reserve((size_t)cap * 4));
    for (DevBuf* d : {&b.qslot, &b.qrank, &b.chunks}) HIP_TRY(c, d->reserve((size_t)cap * nbs * 4));
    HIP_TRY(c, b.binned.reserve((size_t)cap * nbs * 16));
    HIP_TRY(c, b.status.reserve((size_t)cap * nbs)); HIP_TRY(c, b.nbr5.reserve((size_t)cap * nbs * 20));
    HIP_TRY(c, b.nd.reserve((size_t)cap * nbs * 32)); HIP_TRY(c, b.coeff.reserve((size_t)cap * nbs * 8));
    for (DevBuf* d : {&b.bin_key, &b.bin_cnt, &b.bin_off}) HIP_TRY(c, d->reserve((size_t)cap * T * 4));
    HIP_TRY(c, b.partials.reserve((size_t)cap * partial_bytes)); HIP_TRY(c, b.sync.reserve((size_t)cap * kSyncBytes));
    HIP_TRY(c, b.hist.reserve((size_t)cap * kHistReplicas * kHistStride * 4));
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&b.h_states), (size_t)cap * sizeof(DevState)));
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&b.h_begin), (size_t)cap * sizeof(RegBeginArgs)));
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&b.h_active), (size_t)cap * 4));
    // tags / epochs of the record tables and hand-off blocks count up from zero; the state blocks start cleared
    HIP_TRY(c, hipMemsetAsync(b.partials.p, 0, (size_t)cap * partial_bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(b.sync.p, 0, (size_t)cap * kSyncBytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(b.states.p, 0, (size_t)cap * sizeof(DevState), c->stream));
    HIP_TRY(c, hipMemsetAsync(b.hist.p, 0, (size_t)cap * kHistReplicas * kHistStride * 4, c->stream));
    b.cap_hyp = cap; b.bs = nbs; b.table_log2 = lg; b.tables_clean = false;
  }
  if (!b.tables_clean) {  // (bin_offsets leaves the tables empty again)
    HIP_TRY(c, hipMemsetAsync(b.bin_key.p, 0xFF, (size_t)b.cap_hyp * T * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(b.bin_cnt.p, 0, (size_t)b.cap_hyp * T * 4, c->stream));
  }
  return SO_ICP_OK;
}

// so_icp_set_batch_priors: the table of prior blocks of a group (kernels.h: kBatchPriorStride) and its pinned source, for B hypotheses
int batch_priors_reserve(so_icp_ctx* c, uint32_t B) {
  so_icp_ctx::BatchBufs& b = c->batch;
  if (B <= b.cap_prior_hyp) return SO_ICP_OK;
  const uint32_t cap = std::max(B, b.cap_hyp);
  if (b.h_priors) (void)hipHostFree(b.h_priors);
  b.h_priors = nullptr; b.cap_prior_hyp = 0;
  HIP_TRY(c, b.priors.reserve((size_t)cap * kBatchPriorStride * sizeof(double)));
  HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&b.h_priors), (size_t)cap * kBatchPriorStride * sizeof(double)));
  b.cap_prior_hyp = cap;
  return SO_ICP_OK;
}

// `priors`: the priors of the whole batch (so_icp_set_batch_priors; nullptr: none), of which hypothesis h of this group is element base + h
// `keep`: the set this batch leaves (so_icp_keep_batch_correspondences; nullptr: the switch is off), hypothesis h of this group is its base + h
// ---- What a group of so_icp_register_batch and a group of so_icp_match_batch share: the stats headers and the refusals that need no
// launch (batch_group_header), then the group's buffers, prologue arguments, active list, kernel parameters, BatchView, kept-set slice
// and the three binning launches (batch_group_begin).  Behind them the queue holds every hypothesis' prologue and binned scan.
struct BatchGroup {
  std::vector<so_icp_stats> local;  // (the caller passed no stats)
  so_icp_stats* stats = nullptr;
  MatchParams mp; EvalParams ep;    // of the group's sweeps and passes
  BatchView bv{nullptr, nullptr, 0, 0, 0, 0, 0, 0};
  DevState* ds = nullptr;
  CorrBuffers corr{nullptr, nullptr, nullptr};  // (the kernels add the hypothesis' index in the group x bs to these: with the switch on, slice base + h of the kept set)
  uint32_t v_grid = 0;              // workgroups of the single-registration fit pass a hypothesis' workgroups stand in for
};
// -> 1: go on to batch_group_begin; 0: the group is over (hyp_rc says how); < 0: the call is refused
int batch_group_header(so_icp_ctx* c, size_t n, const double* poses_in, int B, double* poses_out /* nullptr: the entry returns no poses */,
                       so_icp_stats* stats, int32_t* hyp_rc, const int pos[3], int count_5x5, BatchGroup& g) {
  if (!stats) { g.local.resize((size_t)B); stats = g.local.data(); }
  g.stats = stats;
  for (int h = 0; h < B; ++h) {
    so_icp_stats* st = stats + h;
    std::memset(st, 0, sizeof(*st));
    st->flags = (!c->dmap ? SO_ICP_FLAG_HOST_MAP : 0u) | (c->direct_readback ? 0u : SO_ICP_FLAG_COPY_READBACK);
    if (poses_out) std::memcpy(poses_out + 7 * (size_t)h, poses_in + 7 * (size_t)h, 7 * sizeof(double));
    fill_stats_header(c, st, pos, count_5x5, n);
    hyp_rc[h] = SO_ICP_OK;
  }
  if (!(count_5x5 > 50)) { for (int h = 0; h < B; ++h) hyp_rc[h] = SO_ICP_NOT_ENOUGH_MAP_FEATURES; return 0; }  // LidarSlam.cpp:113-116
  if (n >= kMaxScanPoints) return refuse_scan_size(c);
  return 1;
}
// `keep`: the set this call leaves (so_icp_keep_batch_correspondences; nullptr: the switch is off), hypothesis h of this group is its base + h
int batch_group_begin(so_icp_ctx* c, const char* entry, const float* d_scan, size_t n, const double* poses_in, int B, int max_outer, int lm_max,
                      int base, so_icp_ctx::KeptSets* keep, BatchGroup& g) {
  const uint32_t lg = bin_table_log2(n);
  const int rc = batch_reserve(c, (uint32_t)B, n, lg);
  if (rc) return rc;
  so_icp_ctx::BatchBufs& b = c->batch;
  hipStream_t s = c->stream;
  for (int h = 0; h < B; ++h) {
    std::memcpy(b.h_begin[h].pose, poses_in + 7 * (size_t)h, 7 * sizeof(double));
    b.h_begin[h].max_outer = max_outer; b.h_begin[h].lm_max = lm_max; b.h_begin[h].chain_expect = 0; b.h_begin[h].pad = 0;  // (a hypothesis starts from its own guess)
    b.h_active[h] = (uint32_t)h;
  }
  HIP_TRY(c, hipMemcpyAsync(b.begin.p, b.h_begin, (size_t)B * sizeof(RegBeginArgs), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(b.active.p, b.h_active, (size_t)B * 4, hipMemcpyHostToDevice, s));
  const float plane_res_now = map_plane_res(c);
  g.mp = match_params(plane_res_now, c->ablate);
  g.mp.chunk_cap = b.bs;
  g.mp.hring[0] = g.mp.hring[1] = nullptr; g.mp.seq_base = 0; g.mp.publish_prev = 0;
  g.mp.packed_leftover = &b.states.as<DevState>()->packed_leftover;
  g.ep = eval_params(plane_res_now, c->cfg.tukey_variant, c->ablate);
  g.ep.n_queries = (uint32_t)n; g.ep.q_stride = 3;
  g.ep.timeout_ticks = 20000000ull;  // 200 ms: a pass of one hypothesis on a few workgroups lasts up to a millisecond
  g.v_grid = solve_grid((uint32_t)n, (uint32_t)c->n_cus);
  g.bv = BatchView{b.active.as<uint32_t>(), b.begin.as<RegBeginArgs>(), b.bs, (uint32_t)((size_t)1 << lg),
                   (uint32_t)((size_t)kFitBlocksMax * kRecordChunksMax * 2), (uint32_t)(kSyncBytes / 4), 1u, g.v_grid};
  const BinTable bt{b.bin_key.as<uint32_t>(), b.bin_cnt.as<uint32_t>(), b.bin_off.as<uint32_t>(), lg};
  g.ds = b.states.as<DevState>();
  // (hypothesis h of the set lies at h * its stride: the last slice of this group is where the kernels will write it)
  if (keep && keep->at[(size_t)(base + B - 1)] != (size_t)(base + B - 1) * b.bs) return fail(c, SO_ICP_E_HIP, std::string(entry) + ": the kept correspondence arrays have another stride than the batch's");
  g.corr = keep ? keep->slice((size_t)base) : CorrBuffers{b.nd.as<double4>(), b.coeff.as<double>(), b.status.as<uint8_t>()};
  if (!n) return SO_ICP_OK;  // (so_icp_match_batch on an empty scan: nothing to bin, its one launch carries the prologue)
  // ---- binning of the scan under every hypothesis' pose: (queries x hypotheses) in three launches
  b.tables_clean = false;
  const double zero_pose[7] = {0, 0, 0, 0, 0, 0, 1};
  launch_scan_keys(d_scan, (uint32_t)n, g.ds, zero_pose, max_outer, lm_max, b.hist.as<int32_t>(), c->view, c->cfg.max_surface_features, 0, 1,
                   b.qslot.as<uint32_t>(), b.qrank.as<uint32_t>(), g.corr.status, bt, s, false, &g.bv, (uint32_t)B);
  launch_bin_offsets(bt, b.chunks.as<uint32_t>(), b.bs, g.ds, s, &g.bv, (uint32_t)B);
  b.tables_clean = true;
  launch_bin_place(bt, d_scan, (uint32_t)n, b.qslot.as<uint32_t>(), b.qrank.as<uint32_t>(), b.binned.as<float4>(), s, nullptr, &g.bv, (uint32_t)B);
  HIP_TRY(c, hipGetLastError());
  return SO_ICP_OK;
}

// `priors`: the priors of the whole batch (so_icp_set_batch_priors; nullptr: none), of which hypothesis h of this group is element base + h
// `keep`: as batch_group_begin's
int register_batch_group(so_icp_ctx* c, const float* d_scan, size_t n, const double* poses_in, int B, double* poses_out, so_icp_stats* stats_io,
                         int32_t* hyp_rc, const int pos[3], int count_5x5, const PriorSet* priors, int base, so_icp_ctx::KeptSets* keep) {
  const auto t_begin = std::chrono::steady_clock::now();
  BatchGroup g;
  int rc = batch_group_header(c, n, poses_in, B, poses_out, stats_io, hyp_rc, pos, count_5x5, g);
  if (rc <= 0) return rc;
  so_icp_stats* const stats = g.stats;
  const int max_outer = outer_limit(c->cfg.max_iterations), lm_max = lm_limit(c->cfg.lm_max_iterations);
  const uint32_t resident_plain = solve_batch_resident_blocks((uint32_t)c->n_cus, c->batch_degrade >= 1 ? 1 : 0);
  // (a round whose list holds a prior launches solve_kernel_batch_prior: ITS occupancy then says how many workgroups are resident together)
  const uint32_t resident_prior = priors ? solve_batch_resident_blocks((uint32_t)c->n_cus, c->batch_degrade >= 1 ? 1 : 0, true) : resident_plain;
  const uint32_t resident = std::min(resident_plain, resident_prior);
  if (resident < (uint32_t)B) {  // (the driver below sizes its groups by the resident workgroups; this is the second line of defence)
    c->err = "so_icp_register_batch: fewer resident solve workgroups (" + std::to_string(resident) + ") than hypotheses in the group (" + std::to_string(B) + ")";
    return kRetryWithoutPersistentSolve;  // degrade (fewer workgroups per hypothesis is not possible: one each) -> concurrent sequential registrations
  }
  if ((rc = batch_group_begin(c, "so_icp_register_batch", d_scan, n, poses_in, B, max_outer, lm_max, base, keep, g))) return rc;
  so_icp_ctx::BatchBufs& b = c->batch;
  hipStream_t s = c->stream;
  const MatchParams& mp = g.mp; const EvalParams& ep = g.ep; BatchView& bv = g.bv; DevState* const ds = g.ds; const CorrBuffers corr = g.corr;
  const uint32_t v_grid = g.v_grid;
  // the hypotheses' priors: one block each, T_meas filled with the hypothesis' guess where its mode says so (the host knows every
  // start pose of a batch); in the queue in front of round 0, so the solve launches read it with plain loads
  std::vector<uint8_t> prior_modes;  // of this group; empty: no hypothesis of it carries a prior
  if (priors) {
    prior_modes.resize((size_t)B);
    bool any = false;
    for (int h = 0; h < B; ++h) any |= (prior_modes[(size_t)h] = (uint8_t)priors->mode(base + h)) != SO_ICP_PRIOR_NONE;
    if (!any) prior_modes.clear();
  }
  if (!prior_modes.empty()) {
    rc = batch_priors_reserve(c, (uint32_t)B);
    if (rc) return rc;
    std::memset(b.h_priors, 0, (size_t)B * kBatchPriorStride * sizeof(double));
    for (int h = 0; h < B; ++h) {
      double* blk = b.h_priors + (size_t)h * kBatchPriorStride;
      PosePrior P;
      if (!priors->frame_prior(base + h, poses_in + 7 * (size_t)h, P)) { blk[6] = 1.0; continue; }  // (mode word 0: nothing else of the block is read)
      std::memcpy(blk, &P, sizeof(P));
      const uint64_t mode_word = prior_modes[(size_t)h];
      std::memcpy(blk + kBatchPriorModeWord, &mode_word, sizeof(mode_word));
      stats[h].flags |= SO_ICP_FLAG_POSE_PRIOR;
    }
    HIP_TRY(c, hipMemcpyAsync(b.priors.p, b.h_priors, (size_t)B * kBatchPriorStride * sizeof(double), hipMemcpyHostToDevice, s));
  }
  std::vector<uint32_t> act((size_t)B);
  for (int h = 0; h < B; ++h) act[(size_t)h] = (uint32_t)h;
  // Rounds are CHAINED -- enqueued on the same list without the host looking at the report in between -- while most of the list is
  // expected to go on: a hypothesis that has finished makes its workgroups of a later round return at once (reg_done), so a stale
  // list costs launches, never results.  After round 0 always (one outer iteration cannot meet the convergence test of most
  // guesses, and a list that shrinks by less than half keeps its workgroups per hypothesis anyway); after a later round when
  // the previous batch of this context found three quarters of that round's list still active (batch_survivors).  Every
  // report + synchronisation left out is 35 us in which the device sits idle (measured: 4 per batch of 5.7 ms).
  for (int it = 0; it < max_outer && !act.empty();) {
    const uint32_t n_act = (uint32_t)act.size();
    if (it > 0) {  // (round 0 uses the identity list uploaded with the poses; the stream was synchronised by the last read-back)
      for (uint32_t k = 0; k < n_act; ++k) b.h_active[k] = act[k];
      HIP_TRY(c, hipMemcpyAsync(b.active.p, b.h_active, (size_t)n_act * 4, hipMemcpyHostToDevice, s));
    }
    // workgroups per hypothesis: the resident grid split evenly (a power of two, never more than the grid they stand in for)
    const bool with_prior = batch_solve_kernel(prior_modes.empty() ? nullptr : prior_modes.data(), act.data(), n_act) == kBatchSolvePrior;
    const uint32_t resident_now = with_prior ? resident_prior : resident_plain;
    uint32_t G = 1;
    while (2u * G * n_act <= resident_now && 2u * G <= v_grid) G *= 2u;
    bv.wg_per_hyp = G;
    const int first = it;
    for (;;) {
      MatchParams mp_it = mp;
      mp_it.skip_near_pass = it == 0 ? 1 : 0;  // round 0 starts with the full k-NN pass (hypotheses +-0.5 m / +-5 degrees off: the near pass certifies almost nothing)
      mp_it.pack_light = (c->knn_pack && !mp_it.skip_near_pass) ? 1 : 0;
      launch_knn_plane(b.binned.as<float4>(), b.chunks.as<uint32_t>(), ds, c->view, mp_it, corr,
                       b.nbr5.as<uint32_t>(), b.hist.as<int32_t>(), s, nullptr, nullptr, &bv, n_act);
      EvalParams ep_it = ep;
      ep_it.epoch_base = (++c->solve_launches) << 5;
      launch_solve_batch(lm_max, d_scan, d_scan + 1, d_scan + 2, corr, ds, ep_it, b.partials.as<double>(), b.sync.as<uint32_t>(), b.hist.as<int32_t>(),
                         c->view, b.nbr5.as<uint32_t>(), mp, bv, n_act, s, with_prior ? b.priors.as<double>() : nullptr);
      HIP_TRY(c, hipGetLastError());
      ++it;
      const bool chain = c->batch_chain && it < max_outer && it - 1 < so_icp_ctx::kBatchRoundsTracked && (it - 1 == 0 || c->batch_survivors[it - 1] >= 0.75f);
      if (!chain) break;
    }
    // at a synchronisation point the host needs two words per hypothesis (outer_iter, reg_done); the whole state blocks (280 KB
    // for 64 hypotheses) are read once, after the last round
    static_assert(offsetof(DevState, reg_done) == offsetof(DevState, outer_iter) + 4, "the round report reads outer_iter and reg_done together");
    HIP_TRY(c, hipMemcpy2DAsync(reinterpret_cast<char*>(b.h_states) + offsetof(DevState, outer_iter), sizeof(DevState),
                                reinterpret_cast<const char*>(ds) + offsetof(DevState, outer_iter), sizeof(DevState), 8, (size_t)B,
                                hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    std::vector<uint32_t> next;
    uint32_t alive_after[so_icp_ctx::kBatchRoundsTracked] = {};
    for (uint32_t h : act) {
      const DevState& H = b.h_states[h];
      // a hypothesis of the list ran the rounds first .. it-1 unless it finished on the way (then outer_iter says where)
      const bool ran_all = H.outer_iter == it, finished_early = H.reg_done && H.outer_iter > first && H.outer_iter < it;
      if (!ran_all && !finished_early) {  // the hypothesis' solve did not finish (a wait inside the launch gave up)
        c->err = "so_icp_register_batch: the solve of hypothesis " + std::to_string(h) + " did not complete in round " + std::to_string(H.outer_iter) +
                 " (workgroups not co-resident: compute units held by another process?)";
        return kRetryWithoutPersistentSolve;
      }
      for (int r = first; r < it && r < so_icp_ctx::kBatchRoundsTracked; ++r)
        if (!(H.reg_done && H.outer_iter <= r + 1)) ++alive_after[r];
      if (!H.reg_done && it < max_outer) next.push_back(h);
    }
    for (int r = first; r < it && r < so_icp_ctx::kBatchRoundsTracked; ++r) c->batch_survivors[r] = (float)alive_after[r] / (float)n_act;
    act.swap(next);
  }
  HIP_TRY(c, hipMemcpyAsync(b.h_states, ds, (size_t)B * sizeof(DevState), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  if ((c->ablate & 128) && c->h_state)  // profiling: so_icp_debug_stamps shows the phase stamps of hypothesis 0's last solve
    for (int i = 0; i < 16; ++i) c->h_state->dbg[i] = b.h_states[0].dbg[i];
  for (int h = 0; h < B; ++h) {
    fill_result(c, b.h_states[h], poses_in + 7 * (size_t)h, stats + h, poses_out + 7 * (size_t)h, false);
    stats[h].time_elapsed_ms = ms;  // (of the whole group: the hypotheses advance together)
    if (!prior_modes.empty() && prior_modes[(size_t)h] != SO_ICP_PRIOR_NONE) stats[h].prediction_source = 1;  // addAbsolutePoseConstraints, LidarSlam.cpp:297
  }
  if (keep) {  // (host memory only: the records themselves are where the kernels wrote them)
    for (int h = 0; h < B; ++h) fill_correspondence_record(keep->rec[(size_t)(base + h)], b.h_states[h], poses_in + 7 * (size_t)h, n, ep);
  }
  return SO_ICP_OK;
}

// so_icp_match_batch: the matching half of one outer iteration and the evaluation at the guess for the B hypotheses of a group -- the
// group's set-up with the bounds of a match (one outer iteration, no LM iteration: plan_registration, icp_context.cpp), round 0's sweep,
// and match_batch_kernel in place of the persistent solve.  One copy of begin arguments + list, 3 + 1 + 1 launches, one copy of the state
// blocks, one synchronisation.  Nothing here waits inside a launch, so the group is as large as the buffers allow whatever is resident.
int match_batch_group(so_icp_ctx* c, const float* d_scan, size_t n, const double* poses, int B, so_icp_stats* stats_io, int32_t* hyp_rc,
                      const int pos[3], int count_5x5, int base, so_icp_ctx::KeptSets* keep) {
  const auto t_begin = std::chrono::steady_clock::now();
  BatchGroup g;
  int rc = batch_group_header(c, n, poses, B, nullptr, stats_io, hyp_rc, pos, count_5x5, g);
  if (rc <= 0) return rc;
  if ((rc = batch_group_begin(c, "so_icp_match_batch", d_scan, n, poses, B, /*max_outer=*/1, /*lm_max=*/0, base, keep, g))) return rc;
  so_icp_ctx::BatchBufs& b = c->batch;
  hipStream_t s = c->stream;
  // the hypotheses' arrival counters (reg_plan.h: match_batch_ticket_word): zero for every call, whatever a launch before left
  static_assert(match_batch_ticket_word(1, kSyncBytes / 4) * 4 == (size_t)kSyncBytes, "one counter at the start of every hypothesis' hand-off block");
  HIP_TRY(c, hipMemset2DAsync(b.sync.p, kSyncBytes, 0, 4, (size_t)B, s));
  if (n) {  // round 0's sweep: the full pass at once (hypotheses +-0.5 m / +-5 degrees off)
    MatchParams mp_it = g.mp;
    mp_it.skip_near_pass = 1; mp_it.pack_light = 0;
    launch_knn_plane(b.binned.as<float4>(), b.chunks.as<uint32_t>(), g.ds, c->view, mp_it, g.corr, b.nbr5.as<uint32_t>(), b.hist.as<int32_t>(), s, nullptr,
                     nullptr, &g.bv, (uint32_t)B);
  }
  launch_match_batch(d_scan, n ? d_scan + 1 : nullptr, n ? d_scan + 2 : nullptr, g.corr, g.ds, g.ep, b.partials.as<double>(), b.sync.as<uint32_t>(), b.hist.as<int32_t>(), c->view,
                     b.nbr5.as<uint32_t>(), g.mp, g.bv, (uint32_t)B, s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(b.h_states, g.ds, (size_t)B * sizeof(DevState), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  for (int h = 0; h < B; ++h) {
    const DevState& H = b.h_states[h];
    if (!H.reg_done || H.n_iterations != 1)
      return fail(c, SO_ICP_E_HIP, "so_icp_match_batch: hypothesis " + std::to_string(base + h) + " was not reported by the device");
    double pose_unused[7];
    fill_result(c, H, poses + 7 * (size_t)h, g.stats + h, pose_unused, false);
    g.stats[h].time_elapsed_ms = ms;  // (of the whole group)
  }
  if (keep) {  // (host memory only: the records themselves are where the kernels wrote them)
    for (int h = 0; h < B; ++h) fill_correspondence_record(keep->rec[(size_t)(base + h)], b.h_states[h], poses + 7 * (size_t)h, n, g.ep);
  }
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_register_batch(so_icp_ctx* c, const float* xyz, const void* d_scan, size_t n, size_t stride_bytes, const double* poses_in,
                          int n_hyp, double* poses_out, so_icp_stats* stats, int32_t* rc_out) {
  if (!c || !poses_in || !poses_out || n_hyp < 0 || (!xyz && !d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (const int rc = refuse_pending(c, "so_icp_register_batch", kPriorsBatch)) return rc;
  if (!c->pending.count_matches(kPriorsBatch, n_hyp)) return fail(c, SO_ICP_E_INVALID, "so_icp_register_batch: n_hyp differs from that of the pending so_icp_set_batch_priors call");
  // so_icp_set_batch_priors: taken out of the context here, so they are consumed whatever this call returns; the group repeats and
  // the fall-back to concurrent registrations below keep them
  const PriorSet batch_priors = c->pending.take(kPriorsBatch);
  const PriorSet* priors = batch_priors.any() ? &batch_priors : nullptr;  // (all NONE: the batch without priors, launch for launch)
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (c->cfg.world_size != 1)  // (hypotheses are independent: replicate the map and split THEM over the ranks -- bench.py's batch64)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_register_batch needs the whole map on one device (world_size == 1)");
  c->corr_last.valid = false;  // (so_icp_correspondences: the hypotheses keep their records in the batch's own arrays)
  if (c->batch_corr) c->batch_corr->valid = false;  // (so_icp_batch_correspondences: this batch replaces the set, or leaves none)
  if (n_hyp == 0) return c->batch_corr_keep ? batch_corr_begin(c, nullptr, n, 0, 0) : 0;
  const float* scan = static_cast<const float*>(d_scan);
  if (!scan) {
    const int rc = upload_scan_impl(c, xyz, n, stride_bytes, c->d_scan_own);
    if (rc) return rc;
    scan = c->d_scan_own.as<float>();
  }
  so_icp_ctx::KeptSets* keep = nullptr;
  if (c->batch_corr_keep) {  // (the stride the groups below will use: batch_reserve never shrinks it)
    if (const int rc = batch_corr_begin(c, scan, n, n_hyp, std::max(batch_stride(n), c->batch.bs))) return rc;
    keep = c->batch_corr.get();
  }
  // the map window is placed once, for hypothesis 0 (LidarSlam.cpp:363); every hypothesis sees that map
  int pos[3];
  map_shift(c, poses_in, pos);
  std::memcpy(c->last_pos, pos, sizeof(pos));
  int rc = upload_map(c);
  if (rc) return rc;
  if (n > 0 && c->batch_degrade < 2) {
    // batched kernels: groups of up to kBatchMaxConcurrent hypotheses advance together (kernels.hip, BatchView)
    const int count = map_count_5x5(c, pos);
    std::vector<int32_t> hrc((size_t)n_hyp, 0);
    for (int base = 0; base < n_hyp;) {
      // a group never holds more hypotheses than solve workgroups can be resident together (one workgroup per hypothesis at
      // least): on a device with few compute units -- SOICP_SOLVE_WORKGROUPS, a partitioned device, one workgroup per unit after
      // a failed co-residency wait -- the batch goes through in smaller groups instead of failing
      uint32_t resident = solve_batch_resident_blocks((uint32_t)c->n_cus, c->batch_degrade >= 1 ? 1 : 0);
      if (priors) resident = std::min(resident, solve_batch_resident_blocks((uint32_t)c->n_cus, c->batch_degrade >= 1 ? 1 : 0, true));
      const int cap = (int)std::min<uint32_t>((uint32_t)kBatchMaxConcurrent, resident);
      if (cap < 1) { c->batch_degrade = 2; break; }
      const int B = std::min(cap, n_hyp - base);
      rc = register_batch_group(c, scan, n, poses_in + 7 * (size_t)base, B, poses_out + 7 * (size_t)base, stats ? stats + base : nullptr,
                                hrc.data() + base, pos, count, priors, base, keep);
      // A batched solve launch needs its workgroups resident together.  If the device could not provide that (shared with another
      // process), the group is repeated with one workgroup per compute unit; if that fails too the context falls back to
      // concurrent sequential registrations (below) for the rest of its life.  so_icp_last_error keeps the notice.
      if (rc == kRetryWithoutPersistentSolve) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->batch.tables_clean = false;
        if (++c->batch_degrade <= 1) continue;  // (the same group again)
        break;
      }
      if (rc < 0) return rc;
      base += B;
    }
    if (c->batch_degrade < 2) {
      int ok = 0;
      for (int h = 0; h < n_hyp; ++h) { if (rc_out) rc_out[h] = hrc[(size_t)h]; if (hrc[(size_t)h] == SO_ICP_OK) ++ok; }
      if (keep) {
        for (int h = 0; h < n_hyp; ++h) keep->rec[(size_t)h].valid = keep->rec[(size_t)h].valid && hrc[(size_t)h] == SO_ICP_OK;
        keep->valid = true;
      }
      return ok;
    }
  }
  // SOICP_BATCH_MODE=lanes, empty scans, and a device that cannot keep the batched solve resident: the hypotheses as concurrent
  // sequential registrations on worker contexts (own stream / buffers / state each, one launch per evaluation)
  const int lanes = std::max(1, std::min(16, n_hyp));
  // worker contexts: own stream / buffers / device state, no map of their own (they borrow this context's resident map)
  while ((int)c->workers.size() < lanes - 1) {
    so_icp_config wc = c->cfg;
    wc.time_kernels = 0;
    so_icp_ctx* w = so_icp_create(&wc);
    if (!w) return fail(c, SO_ICP_E_HIP, "so_icp_register_batch: worker context: " + g_create_error);
    w->dmap.reset();
    c->workers.push_back(w);
  }
  so_icp_ctx::Borrow bw;
  bw.on = true; bw.view = c->view; bw.plane_res = map_plane_res(c);
  std::memcpy(bw.pos, pos, sizeof(pos));
  bw.count_5x5 = map_count_5x5(c, pos);
  std::vector<so_icp_ctx*> lane_ctx(1, c);
  for (int l = 1; l < lanes; ++l) lane_ctx.push_back(c->workers[l - 1]);
  for (so_icp_ctx* w : lane_ctx) {
    w->borrow = bw; w->batch_mode = true; w->batch_single = (lanes == 1);
    std::memcpy(w->prev_obs_hist, c->prev_obs_hist, sizeof(c->prev_obs_hist));
    w->have_hist = c->have_hist; w->startup_count = c->startup_count;
    w->cfg.max_iterations = c->cfg.max_iterations; w->cfg.lm_max_iterations = c->cfg.lm_max_iterations;
    w->cfg.max_surface_features = c->cfg.max_surface_features;
  }
  std::vector<int> lane_rc(lanes, 0);
  std::vector<int> hyp_rc((size_t)n_hyp, 0);
  const EvalParams lane_ep = eval_params(bw.plane_res, c->cfg.tukey_variant, c->ablate);  // (the loss of every lane's registrations)
  if (keep) {  // (groups that ran batched before the context degraded noted theirs: the lanes run every hypothesis again)
    for (so_icp_ctx::CorrLast& r : keep->rec) r.valid = false;
  }
  auto run_lane = [&](int l) {
    so_icp_ctx* w = lane_ctx[l];
    if (hipSetDevice(c->cfg.device_id) != hipSuccess) { lane_rc[l] = SO_ICP_E_HIP; return; }
    for (int h = l; h < n_hyp; h += lanes) {
      so_icp_stats local;
      // P_h becomes the lane context's single prior for this registration, which consumes it (PriorSet::arm: what so_icp_set_pose_prior
      // does, without its refusals); a lane runs one launch per evaluation, eval_kernel_prior
      if (priors) priors->arm(w, h, poses_in + 7 * (size_t)h);
      const PriorOneShot consume{w};
      const int r = register_core(w, scan, n, poses_in + 7 * (size_t)h, poses_out + 7 * (size_t)h, stats ? stats + h : &local);
      hyp_rc[h] = r;
      if (r < 0) { lane_rc[l] = r; return; }
      if (keep && r == SO_ICP_OK) {
        // the lane's context holds this hypothesis' records until its next registration: three copies into slice h on the lane's own
        // queue, behind the registration and in front of the next one
        fill_correspondence_record(keep->rec[(size_t)h], *w->h_state, poses_in + 7 * (size_t)h, n, lane_ep);
        const CorrBuffers to = keep->slice((size_t)h);
        hipError_t e = hipSuccess;
        if (n) e = hipMemcpyAsync(to.nd, w->d_nd.p, n * sizeof(double4), hipMemcpyDeviceToDevice, w->stream);
        if (n && e == hipSuccess) e = hipMemcpyAsync(to.coeff, w->d_coeff.p, n * sizeof(double), hipMemcpyDeviceToDevice, w->stream);
        if (n && e == hipSuccess) e = hipMemcpyAsync(to.status, w->d_status.p, n, hipMemcpyDeviceToDevice, w->stream);
        if (e != hipSuccess) { w->err = std::string("so_icp_register_batch: copy of a lane's correspondences: ") + hipGetErrorString(e); lane_rc[l] = SO_ICP_E_HIP; return; }
      }
    }
    if (keep && hipStreamSynchronize(w->stream) != hipSuccess) { w->err = "so_icp_register_batch: a lane's queue did not drain"; lane_rc[l] = SO_ICP_E_HIP; }
  };
  std::vector<std::thread> th;
  for (int l = 1; l < lanes; ++l) th.emplace_back(run_lane, l);
  run_lane(0);
  for (std::thread& t : th) t.join();
  int ok = 0, err = 0;
  for (int l = 0; l < lanes; ++l) {
    lane_ctx[l]->borrow.on = false; lane_ctx[l]->batch_mode = false;
    if (lane_rc[l] < 0 && !err) { err = lane_rc[l]; if (l > 0) c->err = "worker: " + lane_ctx[l]->err; }
  }
  for (int h = 0; h < n_hyp; ++h) { if (rc_out) rc_out[h] = hyp_rc[h]; if (hyp_rc[h] == SO_ICP_OK) ++ok; }
  if (keep && !err) keep->valid = true;  // (a record is valid where its lane noted it, behind an SO_ICP_OK)
  return err ? err : ok;
}

int so_icp_match_batch(so_icp_ctx* c, const float* xyz, const void* d_scan, size_t n, size_t stride_bytes, const double* poses, int n_poses,
                       so_icp_stats* stats, int32_t* rc_out) {
  if (!c || !poses || !stats || n_poses < 0 || (!xyz && !d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (const int rc = refuse_pending(c, "so_icp_match_batch", kPriorsNone)) return rc;  // (a match takes no prior: whatever is pending stays)
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (c->cfg.world_size != 1) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_match_batch needs the whole map on one device (world_size == 1)");
  // (c->corr_last, the single registration's set, is not this entry's: it stays as it is)
  if (c->batch_corr) c->batch_corr->valid = false;  // (so_icp_batch_correspondences: this call replaces the batch's set, or leaves none)
  if (n_poses == 0) return c->batch_corr_keep ? batch_corr_begin(c, nullptr, n, 0, 0) : 0;
  const float* scan = static_cast<const float*>(d_scan);
  if (!scan && n) {
    const int rc = upload_scan_impl(c, xyz, n, stride_bytes, c->d_scan_own);
    if (rc) return rc;
    scan = c->d_scan_own.as<float>();
  }
  so_icp_ctx::KeptSets* keep = nullptr;
  if (c->batch_corr_keep) {  // (the stride the groups below will use: batch_reserve never shrinks it)
    if (const int rc = batch_corr_begin(c, scan, n, n_poses, std::max(batch_stride(n), c->batch.bs))) return rc;
    keep = c->batch_corr.get();
  }
  // the map window is placed once, for pose 0, as so_icp_register_batch places it; every pose sees that map
  int pos[3];
  map_shift(c, poses, pos);
  std::memcpy(c->last_pos, pos, sizeof(pos));
  if (const int rc = upload_map(c)) return rc;
  const int count = map_count_5x5(c, pos);
  std::vector<int32_t> hrc((size_t)n_poses, 0);
  for (int base = 0; base < n_poses; base += kBatchMaxConcurrent) {
    const int B = std::min(kBatchMaxConcurrent, n_poses - base);
    const int rc = match_batch_group(c, scan, n, poses + 7 * (size_t)base, B, stats + base, hrc.data() + base, pos, count, base, keep);
    if (rc < 0) return rc;
  }
  int ok = 0;
  for (int h = 0; h < n_poses; ++h) { if (rc_out) rc_out[h] = hrc[(size_t)h]; if (hrc[(size_t)h] == SO_ICP_OK) ++ok; }
  if (keep) {
    for (int h = 0; h < n_poses; ++h) keep->rec[(size_t)h].valid = keep->rec[(size_t)h].valid && hrc[(size_t)h] == SO_ICP_OK;
    keep->valid = true;
  }
  return ok;
}

}  // extern "C"
