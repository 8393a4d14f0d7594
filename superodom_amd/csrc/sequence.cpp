// sequence.cpp -- so_icp_register_sequence and so_icp_sequence_announce_next.
//
// A run of scans whose guesses chain: guess_0 = pose0, guess_k = T_(k-1) o delta_k, T_(k-1) = the pose registration k-1 ended with
// (laserMapping.cpp:345-372: T_w_lidar = T_w_lidar * prediction; pose_compose, so_math.h).  Between two so_icp_register calls of a
// stream the device idles for ~11 us: the host reads the last report, returns, is called again and enqueues the first launch of the
// next registration.  Here the NEXT registration's launches are in the queue before the current one has
// reported: the guess is formed on the device, by the solve that ends the registration in front (DevState::T_chain) -- provided the
// registration in front of it was over by then (DevState::done_count): a registration gets `seq_depth` outer iterations enqueued
// ahead (what the last one needed); one that needs more makes the launches behind it no-ops, the host finishes it with further
// launches and starts the next one again, unchained.  Every registration is the one so_icp_register runs from guesses_out[k]: same
// kernels, same arguments, same sums -- identical bits (tests/test_gpu_sequence.py).
// so_icp_set_sequence_priors gives every frame a pose prior of its own: frame k is then so_icp_set_pose_prior(P_k) + so_icp_register,
// P_k's measurement being the frame's guess where the mode says so -- on the device for a chained frame (solve_kernel_prior_at_guess
// reads DevState::pose_in), on the host elsewhere (tests/test_gpu_sequence_priors.py).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

namespace {

// Chained path: single device, device-resident map, persistent solve, direct read-back, yaw_ratio 0 (the stock configurations:
// MannualYawCorrection, LidarSlam.cpp:891-913, is then the identity up to rounding; the chain starts from the optimised pose itself,
// iterations[last].pose_after); everything else -- and SOICP_SEQ_CHAIN=0 -- runs the registrations one after the other with guesses
// composed on the host by the same arithmetic.
bool chained_path(const so_icp_ctx* c, int count, int scans_on_device, size_t stride_bytes) {
  return c->seq_chain && c->dmap && c->cfg.world_size <= 1 && !c->batch_mode && !c->borrow.on && c->persistent_solve && c->direct_readback &&
         c->speculate && c->ablate == 0 && c->cfg.time_kernels <= 1 && c->cfg.yaw_ratio == 0.0 && !c->comm && !c->group && !c->query_split &&
         (scans_on_device || stride_bytes == 12) && count > 1;
}

constexpr int kNotStaged = -1001;  // SequenceCall::stage of an announced scan: not staged ahead (internal: never leaves this file)

struct SeqRun : RegWork {                  // (d_scan, n, query_waves, work list, bounds: what the launches read)
  so_icp_ctx::StageSlot* slot = nullptr;   // host scan (its HBM copy) and / or the work list binned ahead; nullptr: resident scan swept by query waves
  bool binned = false, enqueued = false, chained = false, needs_event = false;
  bool copied = false;                      // the H2D copy of this (host) scan is already in the sequence's queue (issued one registration early)
  bool timed = false;                       // time_kernels 1: this registration's sweeps carry timing events
  struct KnnEv { int it; hipEvent_t a, b; };
  std::vector<KnnEv> knn_ev;
  uint32_t chain_expect = 0;
  double guess[7];                          // exact for an unchained start, the host's prediction for a chained one
  int pos[3] = {0, 0, 0}; int count_5x5 = 0;
  unsigned long long seq_base = 0; int ring = 0; int enq_iters = 0;
  MatchParams mp; EvalParams ep;
  // so_icp_set_sequence_priors: the frame's SO_ICP_PRIOR_* and prior.  AT_GUESS: T_meas is filled by prepare() for a start whose guess
  // the host knows exactly; for a chained start the launches take it from DevState::pose_in (reg_plan.h: sequence_solve_kernel)
  int prior_mode = SO_ICP_PRIOR_NONE;
  PosePrior prior{};
};

// One so_icp_register_sequence call: its arguments, the run record of every scan, what the call before staged for scan 0
struct SequenceCall {
  so_icp_ctx* c; int count; const void* const* scans; const size_t* n_points; size_t stride_bytes; int scans_on_device;
  const double* pose0; const double* deltas; double* poses_out; double* guesses_out; so_icp_stats* stats; int* n_done;
  std::vector<SeqRun> runs;
  PriorSet run_priors;                      // so_icp_set_sequence_priors: taken out of the context when the call started (empty: none were set)
  so_icp_ctx::SeqNext adopted;
  int slot_base = 0;
  bool keep = false;                        // so_icp_keep_sequence_correspondences: this call leaves every frame's set (seq_corr_begin has reserved it)

  const double* delta(int k) const { return deltas + 7 * (size_t)k; }
  // the pose the chain continues from: the optimised pose of the registration, before MannualYawCorrection (fill_result)
  void chain_from(int k, double T[7]) const {
    const so_icp_stats& s = stats[k];
    if (s.n_iterations > 0) std::memcpy(T, s.iterations[std::min(s.n_iterations, SO_ICP_MAX_OUTER) - 1].pose_after, 7 * sizeof(double));
    else std::memcpy(T, poses_out + 7 * (size_t)k, 7 * sizeof(double));
  }
  void exact_guess(int k, double g[7]) const {  // of scan k, once scan k - 1 is done
    if (k == 0) { std::memcpy(g, pose0, 7 * sizeof(double)); return; }
    double T[7];
    chain_from(k - 1, T); pose_compose(T, delta(k), g);
  }
  int run_plain(int k, const double guess[7]) {  // one registration through the ordinary entry points
    if (guesses_out) std::memcpy(guesses_out + 7 * (size_t)k, guess, 7 * sizeof(double));
    run_priors.arm(c, k, guess);  // (the frame's prior, measured at this guess where its mode says so; the entry below consumes it)
    // (keep: the registration copies its scan and the context's records into frame k's slice behind its report, seq_corr_note_plain)
    struct Frame { so_icp_ctx* c; ~Frame() { c->seq_corr_frame = -1; } } frame{c};
    c->seq_corr_frame = keep ? k : -1;
    return scans_on_device ? so_icp_register_dev(c, scans[k], n_points[k], guess, poses_out + 7 * (size_t)k, &stats[k])
                           : so_icp_register(c, static_cast<const float*>(scans[k]), n_points[k], stride_bytes, guess, poses_out + 7 * (size_t)k, &stats[k]);
  }
  int run_unchained() {  // the registrations one after the other, guesses composed on the host
    for (int k = 0; k < count; ++k) {
      double guess[7];
      exact_guess(k, guess);
      const int rc = run_plain(k, guess);
      if (rc) return rc;
      if (n_done) *n_done = k + 1;
    }
    return SO_ICP_OK;
  }

  void init_run(SeqRun& r, size_t n, int k) {  // (k: position in the slot rotation, `count` for the announced scan)
    r.n = n;
    r.query_waves = c->query_waves && query_wave_count_ok(c->cfg.max_surface_features, n, kQueryWaveMaxKept);  // (as register_core_once sweeps it)
    r.ring = (k & 1) * 2;
    r.prior_mode = k < count ? run_priors.mode(k) : SO_ICP_PRIOR_NONE;
    if (r.prior_mode != SO_ICP_PRIOR_NONE) r.prior = run_priors.priors[(size_t)k];
    if (!scans_on_device || !r.query_waves) r.slot = &c->seq_slot[(slot_base + k) % so_icp_ctx::kStageSlots];
    r.max_outer = outer_limit(c->cfg.max_iterations); r.lm_max = lm_limit(c->cfg.lm_max_iterations);
    r.corr = CorrBuffers{c->d_nd.as<double4>(), c->d_coeff.as<double>(), c->d_status.as<uint8_t>()};
    // keep: the frame's sweeps and solves write its slice of the kept set instead -- other kernel arguments, the same kernels.  With
    // so_icp_keep_correspondences on as well the LAST frame writes the context's arrays as it always did (so_icp_correspondences reads
    // them there) and collect() copies them into its slice
    if (keep && k < count && n && !(k == count - 1 && keeps_correspondences(c))) r.corr = c->seq_corr->slice((size_t)k);
  }
  // keep: the packed copy of frame k's scan, on the sequence's own queue behind the scan's arrival and its binning (not on the context's
  // queue, where it would lie between two chained registrations); run_chained waits for that queue before it returns
  int keep_scan(int k) {
    if (!keep) return SO_ICP_OK;
    const SeqRun& r = runs[(size_t)k];
    return seq_corr_copy_scan(c, k, r.d_scan, c->seq_stream);
  }
  int copy_in(SeqRun& r, const void* src) {  // a host scan into its slot, on the sequence's own queue
    if (r.copied) return SO_ICP_OK;
    HIP_TRY(c, r.slot->dev.reserve((r.n + 64) * 12));
    HIP_TRY(c, hipMemcpyAsync(r.slot->dev.p, src, r.n * 12, hipMemcpyHostToDevice, c->seq_stream));
    r.copied = true;
    return SO_ICP_OK;
  }
  // the scan's way to HBM and its work list, on the sequence's own queue: copy (host scans), scan_keys -> bin_offsets -> bin_place under
  // `pose` (scans swept in chunks), one event.  Slot k % 3: its last user, scan k - 3, was collected before scan k - 1 was enqueued.
  // `announced`: the scan that will start the NEXT call (so_icp_sequence_announce_next), staged beside this call's last registration.
  // For that one any return but SO_ICP_OK only means "not staged ahead" (stage_announced), and the hash table is taken as the last
  // binning of this call left it -- clean at this size, or not used: never re-ensured or cleared under the registrations in flight.
  int stage(SeqRun& r, const void* src, const double pose[7], bool announced) {
    r.d_scan = static_cast<const float*>(src);
    r.binned = false; r.needs_event = false;
    if (!r.slot || !r.n) { if (!scans_on_device) r.d_scan = nullptr; return announced ? kNotStaged : SO_ICP_OK; }
    so_icp_ctx::StageSlot& sl = *r.slot;
    if (!sl.ev) HIP_TRY(c, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
    if (!scans_on_device) {
      const int rc = copy_in(r, src);
      if (rc) return rc;
      r.d_scan = sl.dev.as<float>();
      r.needs_event = true;
    }
    if (!r.query_waves) {
      if (!c->prebin) return SO_ICP_OK;  // (binned by the registration itself: never chained)
      HIP_TRY(c, sl.reserve_worklist(r.n));
      if (announced) { if (c->sbin.log2 != bin_table_log2(r.n)) return kNotStaged; }
      else HIP_TRY(c, c->sbin.ensure(bin_table_log2(r.n), c->seq_stream));
      if (!bin_into_slot(c, r.d_scan, r.n, pose, c->seq_stream, c->sbin, sl)) return fail(c, SO_ICP_E_HIP, "so_icp_register_sequence: the binning launches were refused");
      r.binned = true; r.needs_event = true;
      r.d_binned = sl.pb_binned.as<float4>(); r.d_chunks = sl.pb_chunks.as<uint32_t>();
    }
    if (r.needs_event) HIP_TRY(c, hipEventRecord(sl.ev, c->seq_stream));
    return SO_ICP_OK;
  }
  // The copy of a host scan TWO registrations ahead (its slot's last user, scan k - 3, has been collected): the binning of scan k + 1 is then
  // enqueued with its scan long in HBM and runs beside the FIRST SWEEP of registration k -- hundreds of short wavefronts next to a sweep that
  // leaves 60 % of its issue slots empty -- instead of behind a 34 us copy, beside the first solve, whose one wavefront per SIMD it slowed
  // by ~5 us (41 - 43 us against 36 - 37 for the second solve of the same registration: profiles/r06/sequence_timeline_flag_wait.txt).
  int copy_ahead(int k) {
    if (k >= count || scans_on_device) return SO_ICP_OK;
    SeqRun& r = runs[(size_t)k];
    return (r.slot && r.n) ? copy_in(r, scans[k]) : SO_ICP_OK;
  }
  // the host's prediction of the guess of the scan BEHIND registration k, formed while k runs (k - 1 has been collected on every path
  // by then: chained, after a chain break, after run_plain): anchored on k's exact guess, never on the prediction k was started under
  void predict_next(int k, const double delta_next[7], double pred[7]) const {
    double g[7];
    exact_guess(k, g);
    predicted_guess(g, delta_next, pred);
  }
  // the scan that will start the NEXT call: on its way to HBM and binned beside this call's last registration
  void stage_announced() {
    so_icp_ctx::SeqNext& nx = c->seq_next;
    nx.announced = false;
    double pred[7];
    predict_next(count - 1, nx.delta, pred);
    nx.scan = nx.next_scan; nx.n = nx.next_n;
    nx.slot = (slot_base + count) % so_icp_ctx::kStageSlots;
    SeqRun rn;
    init_run(rn, nx.n, count);
    std::string err = c->err;  // (a failure is no error of this call: neither its return value nor its text)
    nx.staged = stage(rn, nx.scan, pred, true) == SO_ICP_OK;
    if (!nx.staged) c->err.swap(err);
    (void)hipGetLastError();
    nx.binned = rn.binned; nx.needs_event = rn.needs_event; nx.d_scan = nx.staged ? rn.d_scan : nullptr;
  }
  // host side of a registration's start (register_core_once): window, map view, parameters.  false + rc == 0: cannot be started this way
  bool prepare(int k, const double guess[7], bool chained, int* rc_out) {
    SeqRun& r = runs[(size_t)k];
    *rc_out = SO_ICP_OK;
    std::memcpy(r.guess, guess, sizeof(r.guess));
    if (r.prior_mode == SO_ICP_PRIOR_AT_GUESS && !chained) std::memcpy(r.prior.T_meas, guess, sizeof(r.prior.T_meas));  // (exact: the BEGIN launch starts from this argument)
    if (!r.query_waves && !r.binned) return false;
    if (!c->no_map_shift) {
      const int dims[3] = {kMapW, kMapH, kMapD};
      if (chained && !cube_stable(map_origin(c), dims, guess, 1.0)) return false;
      map_shift(c, guess, r.pos); std::memcpy(c->last_pos, r.pos, sizeof(r.pos));
    } else std::memcpy(r.pos, c->last_pos, sizeof(r.pos));
    r.count_5x5 = map_count_5x5(c, r.pos);
    if (!(r.count_5x5 > 50)) { if (!chained) *rc_out = SO_ICP_NOT_ENOUGH_MAP_FEATURES; return false; }  // LidarSlam.cpp:113-116
    if ((*rc_out = upload_map(c))) return false;
    r.seq_base = registration_params(c, map_plane_res(c), r.n, r.binned ? r.slot->pb_chunk_cap : 0, r.ring, r.mp, r.ep);
    r.chained = chained;
    // (every seventh registration -- a period coprime to the scan rotation of the benchmarks: an event pair on a dispatch was measured at
    //  ~8 us of queue time here, where no idle moment between back-to-back chained launches hides it: 4 % of the rate at every third)
    r.timed = c->cfg.time_kernels == 1 && (k % 7) == 0;
    r.knn_ev.clear();
    r.chain_expect = chained ? c->done_count_seen + 1u : 0u;  // (exactly the registration in front of this one completes in between)
    r.mp.chain_expect = r.chain_expect; r.ep.chain_expect = r.chain_expect;
    return true;
  }
  // outer iterations [it0, it1) of run k into the queue; the solve of it1 - 1 reports by itself (nothing of this registration is
  // enqueued behind it yet), the others leave their report to the sweep behind them (EvalParams::defer_publish)
  int enqueue(int k, int it0, int it1) {
    SeqRun& r = runs[(size_t)k];
    // Scan and work list come from the other queue.  The host WATCHES that queue's event for the scan (the copy went out a registration
    // ago, the binning a moment ago: tens of microseconds, and the registration in front has only just begun) and enqueues this
    // registration's launches once it has fired -- then nothing has to order the two queues on the device.  Measured alternatives: a
    // barrier packet in front of the first launch (hipStreamWaitEvent) costs 5.6 us of command-processor time between two registrations;
    // a first launch that polls a flag in device memory costs nothing -- and deadlocks when it is dispatched before the binning
    // kernels it waits for (its 4 096 spinning wavefronts fill the chip: seen once, on a first call whose allocations had held the host up).
    if (it0 == 0 && r.needs_event) {
      const auto t_w = std::chrono::steady_clock::now();
      bool fired = false;
      for (unsigned spin = 0;; ++spin) {
        const hipError_t q = hipEventQuery(r.slot->ev);
        if (q == hipSuccess) { fired = true; break; }
        if (q != hipErrorNotReady) break;
        if ((spin & 15u) == 15u && std::chrono::steady_clock::now() - t_w > std::chrono::microseconds(400)) break;
      }
      (void)hipGetLastError();
      if (!fired) HIP_TRY(c, hipStreamWaitEvent(c->stream, r.slot->ev, 0));  // (the other queue is late: let the device order the two)
    }
    for (int it = it0; it < it1; ++it) {
      MatchParams mp_it = r.mp;
      mp_it.publish_prev = (it > it0) ? 1 : 0;  // (the solve in front of this sweep deferred its report)
      hipEvent_t ka = nullptr, kb = nullptr;
      if (r.timed) {  // (the events ride on the dispatch packet, no marker packets)
        ka = next_event(c); kb = next_event(c);
        if (ka && kb) r.knn_ev.push_back(SeqRun::KnnEv{it, ka, kb}); else ka = kb = nullptr;
      }
      launch_sweep(c, r, mp_it, it == 0, it == 0 ? r.slot : nullptr, r.guess, r.chain_expect, ka, kb);
      EvalParams ep_it = r.ep;
      ep_it.defer_publish = (it + 1 < it1) ? 1 : 0;
      if (k + 1 < count) { ep_it.chain_next = 1; std::memcpy(ep_it.chain_delta, delta(k + 1), sizeof(ep_it.chain_delta)); }  // (whichever solve ends this registration forms the next guess)
      const SolveKernelKind kind = sequence_solve_kernel(r.prior_mode, r.chained);
      launch_persistent_solve(c, r, ep_it, r.mp, kind == kSolvePlain ? nullptr : &r.prior, kind == kSolvePriorAtGuess);
    }
    HIP_TRY(c, hipGetLastError());
    r.enq_iters = it1; r.enqueued = true;
    return SO_ICP_OK;
  }
  // prepare, then the iterations a registration gets enqueued ahead: what the last one needed (so_icp_ctx::seq_depth)
  bool start(int k, const double guess[7], bool chained, int* rc_out) {
    if (!prepare(k, guess, chained, rc_out)) return false;
    *rc_out = enqueue(k, 0, std::max(1, std::min(c->seq_depth, runs[(size_t)k].max_outer)));
    return true;
  }
  int await(int k, int it) {
    const SeqRun& r = runs[(size_t)k];
    const Report rep = await_report(c, &c->h_ring[r.ring + (it & 1)]->seq, r.seq_base | (unsigned long long)(it + 1), c->stream);
    if (rep != Report::kDrained) return rep == Report::kReported ? SO_ICP_OK : SO_ICP_E_HIP;
    return fail(c, SO_ICP_E_HIP, "so_icp_register_sequence: registration state was not published by the device");
  }
  // the results of run k, reported last by outer iteration `last`
  int collect(int k, int last, std::chrono::steady_clock::time_point t_icp) {
    SeqRun& r = runs[(size_t)k];
    so_icp_stats* st = &stats[k];
    // (a registration swept by query waves builds no work list: knn_list_fits stays; the state block is the context's own)
    note_registration_done(c, c->h_ring[r.ring + (last & 1)], r.mp, r.n, !r.query_waves, true);
    const DevState& H = *c->h_state;
    std::memset(st, 0, sizeof(*st));
    st->flags = (r.slot && !scans_on_device ? SO_ICP_FLAG_STAGED_SCAN : 0u) | (r.binned ? SO_ICP_FLAG_BINNED_AHEAD : 0u) |
                (r.query_waves ? SO_ICP_FLAG_QUERY_WAVES : 0u) | (r.chained ? SO_ICP_FLAG_CHAINED : 0u) |
                (r.prior_mode != SO_ICP_PRIOR_NONE ? SO_ICP_FLAG_POSE_PRIOR : 0u);
    fill_stats_header(c, st, r.pos, r.count_5x5, r.n);
    double guess[7];
    std::memcpy(guess, H.pose_in, sizeof(guess));  // (what the device formed for a chained registration; the host's own argument otherwise)
    if (guesses_out) std::memcpy(guesses_out + 7 * (size_t)k, guess, sizeof(guess));
    c->seq_depth = std::max(1, H.n_iterations);
    for (const SeqRun::KnnEv& e : r.knn_ev) {  // sweeps that did real work (a launch behind the converged iteration was a no-op); they ended long ago
      float ms = 0;
      if (e.it < H.n_iterations && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
        c->timing.knn_ms_total += ms; c->timing.knn_launches++;
        c->timing.knn_queries += r.query_waves ? (int64_t)r.n : (int64_t)work_list_kept(H.bin_packed); c->timing.knn_map_points += c->view.n_points;
      }
    }
    (void)hipGetLastError();
    fill_result(c, H, guess, st, poses_out + 7 * (size_t)k, true);
    if (r.prior_mode != SO_ICP_PRIOR_NONE) st->prediction_source = 1;  // addAbsolutePoseConstraints, LidarSlam.cpp:297
    if (keep) seq_corr_note(c, k, H, guess, r.ep);  // (so_icp_sequence_correspondences: this frame's record; its slice holds its last fit pass)
    if (k == count - 1 && keeps_correspondences(c)) {
      // so_icp_correspondences exports the LAST registration of the run (the context's arrays hold the records of no other: the launches
      // chained behind a frame overwrite them; the sets of ALL frames: so_icp_keep_sequence_correspondences).  Its scan lies in a slot the next call refills on the sequence's own queue: copied now, and waited for
      if (const int rc = keep_scan_copy(c, r.d_scan, r.n)) return rc;
      const bool geometry = keeps_correspondence_geometry(c);  // (so_icp_correspondence_geometry: its snapshot, in front of the same wait)
      if (geometry) { if (const int rc = keep_neighbour_snapshot(c, r.n)) return rc; }
      if (keep) { if (const int rc = seq_corr_copy_records(c, k)) return rc; }  // (both switches on: this frame wrote the context's arrays)
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      note_correspondences(c, H, guess, r.n, r.ep);
      if (geometry) note_correspondence_geometry(c, r.mp);
    }
    st->time_elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_icp).count();
    c->timing.registrations++;
    if (r.chained) {
      c->timing.seq_chained++;
      // the window was placed for the predicted guess: the actual one must lie in the same block (cube_stable saw to it)
      const int* o = map_origin(c);
      if (cube_coord(guess[0], o[0]) != r.pos[0] || cube_coord(guess[1], o[1]) != r.pos[1] || cube_coord(guess[2], o[2]) != r.pos[2])
        return fail(c, SO_ICP_E_HIP, "so_icp_register_sequence: a chained guess left the map block its window was placed for");
    }
    return SO_ICP_OK;
  }

  int run_chained() {
    if (!c->seq_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->seq_stream, hipStreamNonBlocking));
    struct Drain {  // an early return must not leave copies reading the caller's buffers, nor launches of this call in the queue
      so_icp_ctx* c; bool ok = false;
      ~Drain() { if (!ok) { (void)hipStreamSynchronize(c->seq_stream); (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); c->ev_used = 0; } }
    } drain{c};
    size_t n_max = 0;
    for (int k = 0; k < count; ++k) {
      if (n_points[k] >= kMaxScanPoints) return refuse_scan_size(c);
      n_max = std::max(n_max, n_points[k]);
    }
    int rc = SO_ICP_OK;
    if ((rc = reserve_scan_buffers(c, n_max))) return rc;  // (once, for the longest scan: nothing is re-allocated under a registration in flight)
    if ((rc = upload_map(c))) return rc;                   // (the binning ahead of scan 0 reads the map view before the first prepare())
    // scan 0 may already be in HBM with its work list: the call before this one staged it beside its last registration (so_icp_sequence_announce_next)
    adopted = c->seq_next;
    const bool adopt = adopted.staged && adopted.scan == scans[0] && adopted.n == n_points[0];
    slot_base = adopt ? adopted.slot : 0;
    c->seq_next.staged = false;
    runs.resize((size_t)count);
    for (int k = 0; k < count; ++k) init_run(runs[(size_t)k], n_points[k], k);
    // scan 0: an ordinary start from pose0
    if (adopt) {
      SeqRun& r0 = runs[0];
      r0.d_scan = adopted.d_scan; r0.binned = adopted.binned; r0.needs_event = adopted.needs_event;
      if (r0.binned) { r0.d_binned = r0.slot->pb_binned.as<float4>(); r0.d_chunks = r0.slot->pb_chunks.as<uint32_t>(); }
    } else if ((rc = stage(runs[0], scans[0], pose0, false))) return rc;
    if ((rc = keep_scan(0))) return rc;
    if ((rc = copy_ahead(1))) return rc;
    bool started = start(0, pose0, false, &rc);
    if (rc) return rc;
    for (int k = 0; k < count; ++k) {
      SeqRun& r = runs[(size_t)k];
      bool next_started = false;
      if (!started) {
        // this scan cannot be started from here (an empty scan, too little map, a window about to roll, ...): the ordinary entry point,
        // from the guess the chain arithmetic gives -- same results, and the next scan starts a new chain
        double guess[7];
        exact_guess(k, guess);
        if (hipStreamSynchronize(c->seq_stream) != hipSuccess) return fail(c, SO_ICP_E_HIP, "so_icp_register_sequence: copy queue");
        if ((rc = run_plain(k, guess))) return rc;
        if (n_done) *n_done = k + 1;
        if (k + 1 < count) {  // (after a plain registration: the next scan starts a chain of its own)
          double g[7];
          exact_guess(k + 1, g);
          if ((rc = stage(runs[(size_t)k + 1], scans[k + 1], g, false))) return rc;
          if ((rc = keep_scan(k + 1))) return rc;
          started = start(k + 1, g, false, &rc);
          if (rc && rc != SO_ICP_NOT_ENOUGH_MAP_FEATURES) return rc;
        }
        continue;
      }
      const auto t_icp = std::chrono::steady_clock::now();
      // the NEXT scan: on its way to HBM, binned under the host's prediction of its guess, and -- the point of this entry -- its
      // registration enqueued behind this one's launches
      if (k + 1 < count) {
        double pred[7];
        // exact_guess(k) o delta_(k+1), NOT r.guess o delta_(k+1): r.guess of a chained registration is itself a prediction, and a chain of
        // predictions gathers the correction of every frame since the call began (metres after a few hundred frames: chunks that
        // straddle cells, then a window refused by cube_stable).  This registration moves its exact guess by centimetres: good enough
        // to bin under and to place the window, and no worse at frame 1 000 than at frame 1
        predict_next(k, delta(k + 1), pred);
        if ((rc = stage(runs[(size_t)k + 1], scans[k + 1], pred, false))) return rc;
        if ((rc = keep_scan(k + 1))) return rc;
        if ((rc = copy_ahead(k + 2))) return rc;
        next_started = start(k + 1, pred, true, &rc);
        if (rc) return rc;
      } else if (c->seq_next.announced && !scans_on_device) {
        stage_announced();
      }
      // this registration's reports
      int last = 0;
      for (int it = 0;; ++it) {
        if ((rc = await(k, it))) return rc;
        last = it;
        if (c->h_ring[r.ring + (it & 1)]->reg_done || it + 1 >= r.max_outer) break;
        if (it + 1 >= r.enq_iters) {
          // it needs more outer iterations than were enqueued ahead: the chained registration behind it has found it unfinished
          // and turned itself off (DevState::done_count); one iteration at a time from here, the next scan starts again afterwards
          if (next_started) { next_started = false; runs[(size_t)k + 1].enqueued = false; c->timing.seq_chain_breaks++; }
          if ((rc = enqueue(k, it + 1, it + 2))) return rc;
        }
      }
      if ((rc = collect(k, last, t_icp))) return rc;
      if (k + 1 < count && !next_started && !runs[(size_t)k + 1].enqueued) {
        // an ordinary start of the next scan, from the exact guess (after a broken chain: its copy and work list are where they were)
        double g[7];
        exact_guess(k + 1, g);
        next_started = start(k + 1, g, false, &rc);
        if (rc && rc != SO_ICP_NOT_ENOUGH_MAP_FEATURES) return rc;
      }
      started = next_started;
      if (n_done) *n_done = k + 1;
    }
    c->scan_staged = false;
    c->ev_used = 0;  // (the timing events of this call are free again)
    if (keep) HIP_TRY(c, hipStreamSynchronize(c->seq_stream));  // (the scan copies of the kept set)
    drain.ok = true;
    return SO_ICP_OK;
  }
};

}  // namespace

extern "C" {

int so_icp_sequence_announce_next(so_icp_ctx* c, const float* scan, size_t n, const double delta[7]) {
  if (!c || (scan && !delta)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  so_icp_ctx::SeqNext& nx = c->seq_next;
  if (!scan || !n) {  // withdrawn: the announcement, and a copy the last call staged (which must have left its buffer before the caller reuses it)
    if (nx.staged && c->seq_stream) { HIP_TRY(c, hipSetDevice(c->cfg.device_id)); HIP_TRY(c, hipStreamSynchronize(c->seq_stream)); }
    nx = so_icp_ctx::SeqNext{};
    return SO_ICP_OK;
  }
  // (what the LAST call staged for the coming call to adopt -- nx.staged and its slot -- stays: this names the scan BEHIND the coming call)
  nx.next_scan = scan; nx.next_n = n; nx.announced = true;
  std::memcpy(nx.delta, delta, sizeof(nx.delta));
  return SO_ICP_OK;
}

int so_icp_register_sequence(so_icp_ctx* c, int count, const void* const* scans, const size_t* n_points, size_t stride_bytes, int scans_on_device,
                             const double pose0[7], const double* deltas, double* poses_out, double* guesses_out, so_icp_stats* stats, int* n_done) {
  if (n_done) *n_done = 0;
  if (!c || count < 0 || (count && (!scans || !n_points || !pose0 || !poses_out)) || (count > 1 && !deltas)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (const int rc = refuse_pending(c, "so_icp_register_sequence", kPriorsRun)) return rc;
  // so_icp_set_sequence_priors: one prior per frame of THIS call -- a call of another length leaves them pending, this one takes them
  // out of the context (consumed whatever it returns; the per-frame entries it may run do not meet them)
  if (!c->pending.count_matches(kPriorsRun, count)) return fail(c, SO_ICP_E_INVALID, "so_icp_register_sequence: count differs from that of the pending so_icp_set_sequence_priors call");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  if (stride_bytes == 0) stride_bytes = 12;
  for (int k = 0; k < count; ++k) if (!scans[k] && n_points[k]) return SO_ICP_E_INVALID;
  // so_icp_keep_sequence_correspondences: the set of this run, reserved here -- before the run's first launch, and before the call has
  // touched anything (SO_ICP_E_NOMEM leaves the priors pending and the last registration's set valid)
  const bool keep = keeps_sequence_correspondences(c);
  if (keep) { if (const int rc = seq_corr_begin(c, count, n_points)) return rc; }
  PriorSet run_priors = c->pending.take(kPriorsRun);
  std::vector<so_icp_stats> local_stats;
  if (!stats) { local_stats.resize((size_t)count); stats = local_stats.data(); }
  SequenceCall call{c, count, scans, n_points, stride_bytes, scans_on_device, pose0, deltas, poses_out, guesses_out, stats, n_done};
  call.run_priors = std::move(run_priors);
  c->corr_last.valid = false;
  call.keep = keep && c->seq_corr->valid;
  const int rc = chained_path(c, count, scans_on_device, stride_bytes) ? call.run_chained() : call.run_unchained();
  if (rc != SO_ICP_OK) c->corr_last.valid = false;  // (so_icp_correspondences: only a run that completed leaves its last registration's set)
  if (rc < 0 && call.keep) seq_corr_fail(c);        // (so_icp_sequence_correspondences: a run that failed leaves no frame's set)
  return rc;
}

}  // extern "C"
