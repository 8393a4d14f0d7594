// ctx.h -- the host driver's context (struct so_icp_ctx) and the helpers its translation units share.  Private to libsoicp: the
// C ABI (include/so_icp.h) sees the context as an opaque handle.  The entry points live by family:
//   icp_context.cpp       create / destroy / configuration, the map entries, so_icp_register(_dev) and the registration itself
//   staging.cpp           so_icp_stage_scan: slots, copy thread, binning ahead, so_icp_host_register / _alloc
//   sequence.cpp          so_icp_register_sequence, so_icp_sequence_announce_next
//   batch.cpp             so_icp_register_batch
//   reg_plan.h            what all three decide without a device: loop limits, query split, table and work-list sizes, window rule
//   localization.cpp      so_icp_localization(_dev): one frame of LidarSLAM::Localization from a host or a resident scan
//   prefilter.cpp         so_icp_prefilter_announce / _scan(_dev): adjustVoxelSize + VoxelGrid, decided on the device or on the host
//   cloud_steps.cpp       so_icp_deskew_scan(_dev), so_icp_transform_cloud, so_icp_download_scan
//   correspondences.cpp   so_icp_keep_correspondences, so_icp_correspondences: the last registration's correspondence set;
//                         so_icp_match(_dev), so_icp_correspondence_sums: the set formed at a pose of the caller's, its sums on the device
//                         so_icp_keep_correspondence_geometry, so_icp_correspondence_geometry: its neighbours, PCA and observability labels
//   pose_prior.cpp        so_icp_pose_prior_from_information, so_icp_pose_prior_sums, so_icp_set_pose_prior, so_icp_set_sequence_priors,
//                         so_icp_set_batch_priors
//   selection_correspondences.cpp   the correspondence sets of a batch's hypotheses and of a run's frames: the switches, what the
//                         batch and sequence entries keep while they are on, the exports and sums of both over one host path
//   multi_gpu.cpp         RCCL, in-process groups, peer exchange, shard helpers
//   localization_sequence.cpp, feature_extraction.cpp
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/so_icp.h"
#include "device_map.h"
#include "kernels.h"
#include "local_map.h"
#include "lm_solver.h"
#include "reg_plan.h"
#include "so_math.h"

namespace soicp::host {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
  template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// A pinned host buffer that grows (the tables and read-backs of the batch and sequence correspondence exports)
struct PinnedBuf {
  uint8_t* p = nullptr;
  size_t cap = 0;
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 4 + 256;
    const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  ~PinnedBuf() { if (p) (void)hipHostFree(p); }
};

// RCCL entry points: prototypes and types come from <rccl/rccl.h>; the library itself is resolved lazily with dlopen
// (a single-GPU process never loads librccl -- one collective per evaluation is the only use)
struct Rccl {
  void* lib = nullptr;
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclAllReduce) AllReduce = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
static_assert(sizeof(ncclUniqueId) == SO_ICP_UNIQUE_ID_BYTES, "SO_ICP_UNIQUE_ID_BYTES must equal sizeof(ncclUniqueId)");

struct EventSpan { int kind; hipEvent_t a, b; uint32_t units; };  // kind 0 knn, 1 eval, 2 prep

// The hash table of a scan's binning (scan_keys -> bin_offsets -> bin_place): keys, counts, offsets of 2^log2 slots.  bin_offsets
// leaves it empty again, so it is cleared (keys 0xFF, counts 0) only when it is new, changes size, or a binning did not complete.
struct BinHashTable {
  DevBuf key, cnt, off;
  uint32_t log2 = 0;  // of the table as it stands clean; 0: clear before the next use
  bool fits(uint32_t lg) const { const size_t b = (size_t)4 << lg; return key.cap >= b && cnt.cap >= b && off.cap >= b; }
  hipError_t reserve(uint32_t lg) {  // (a table that moves is cleared again before its next use)
    if (fits(lg)) return hipSuccess;
    log2 = 0;
    const size_t b = (size_t)4 << lg;
    hipError_t e = key.reserve(b);
    if (e == hipSuccess) e = cnt.reserve(b);
    if (e == hipSuccess) e = off.reserve(b);
    return e;
  }
  // reserve (a no-op when the table fits) and clear, unless the table stands clean at this size
  hipError_t ensure(uint32_t lg, hipStream_t s) {
    if (log2 == lg) return hipSuccess;
    log2 = 0;
    hipError_t e = reserve(lg);
    if (e == hipSuccess) e = hipMemsetAsync(key.p, 0xFF, (size_t)4 << lg, s);
    if (e == hipSuccess) e = hipMemsetAsync(cnt.p, 0, (size_t)4 << lg, s);
    if (e == hipSuccess) log2 = lg;
    return e;
  }
  BinTable view() const { return BinTable{key.as<uint32_t>(), cnt.as<uint32_t>(), off.as<uint32_t>(), log2}; }
  void release() { key.release(); cnt.release(); off.release(); log2 = 0; }
};
static_assert(kOuterCap == SO_ICP_MAX_OUTER, "outer_limit (reg_plan.h) caps at the per-iteration statistics of so_icp_stats");

struct InprocGroup;  // so_icp_comm_init_inprocess (multi_gpu.cpp)

// Life of a stage slot (so_icp_stage_scan, staging.cpp): empty -> (queued: the copy thread owns it) -> ready -> in use by the registration
// that consumes it -> empty; failed: the copy thread's error waits in the slot for the call that asks for the scan
enum class StageState : int { kFailed = -1, kEmpty = 0, kQueued = 1, kReady = 2, kInUse = 3 };

}  // namespace soicp::host

// (the context is the C ABI's global struct; these name the driver's types in it and in every translation unit that includes this header)
using namespace soicp;
using namespace soicp::host;

struct so_icp_ctx {
  so_icp_config cfg;
  std::string err;
  bool host_only = false;  // device_id < 0: LocalMap bookkeeping only, every compute entry point fails
  LocalMap map;                     // host LocalMap: host-only contexts and sharded (world_size > 1) contexts
  std::unique_ptr<DeviceMap> dmap;  // HBM-resident LocalMap with GPU insert (world_size == 1)
  DevBuf d_world;                   // world-frame copy of the scan for the map insert
  CanonicalMap cm;
  uint64_t uploaded_version = 0;
  hipStream_t stream = nullptr;
  // map shard in HBM
  DevBuf d_mpts, d_cell_start, d_cube_slot;
  DevMapView view{};
  // scan / correspondence buffers
  DevBuf d_scan_own, d_keys0, d_vals0, d_chunks, d_binned, d_nd, d_coeff, d_status, d_nbr5;
  DevBuf d_kdbg;   // profiling only
  DevBuf d_counts; // sharded device map: per-cube counters on their way through the all-reduce
  DevBuf d_small;  // hist[16] int32 | ticket | n_kept | fb_count | LmSums | partials
  int32_t* d_hist = nullptr; uint32_t* d_ticket = nullptr; uint32_t* d_nkept = nullptr; uint32_t* d_fbcount = nullptr;
  LmSums* d_sums = nullptr; double* d_partials = nullptr;
  LmSums* h_sums = nullptr; uint32_t* h_u32 = nullptr;  // pinned
  DevBuf d_state_buf; DevState* d_state = nullptr; DevState* h_state = nullptr;  // device-resident registration state + the pinned mirror read last
  // per-outer-iteration read-backs (double-buffered); mirrors 2, 3: the second pair of so_icp_register_sequence, whose chained
  // registrations alternate between the pairs (the next registration starts reporting before the host has read the last report of this one)
  DevState* h_ring[4] = {nullptr, nullptr, nullptr, nullptr}; hipEvent_t ev_outer[2] = {nullptr, nullptr};
  DevState* d_ring[4] = {nullptr, nullptr, nullptr, nullptr};  // device-side addresses of the pinned mirrors
  bool direct_readback = true; unsigned long long reg_counter = 0;
  bool persistent_solve = true;  // SOICP_PERSISTENT=0: one launch per evaluation
  unsigned long long solve_launches = 0;  // persistent solve launches so far (EvalParams::epoch_base)
  BinHashTable bin;  // the registration's own binning
  int32_t* h_hist = nullptr;  // pinned: per-outer-iteration copy of the histogram replicas (profiling mode)
  std::vector<DevBuf> resident_scans;  // so_icp_upload_scan
  // so_icp_prefilter_announce: the NEXT raw cloud, already on its way to HBM (pf_stage) when so_icp_prefilter_scan is called with the same buffer
  DevBuf pf_stage; std::mutex pf_mu, aux_mu;
  struct PfAnnounced { const void* ptr = nullptr; size_t n = 0, stride = 0; bool on = false; } pf_announced;
  DevBuf pf_in, pf_out, pf_small, pf_w, pf_s, pf_k0, pf_k1, pf_v0, pf_v1, pf_flags, pf_pos, pf_heads, pf_temp;  // so_icp_prefilter_scan
  DevBuf pf_dec;                      // {counters[16], VgDecision, partial statistics}: the pre-filter decided on the device
  VgDecision* h_pf = nullptr;         // pinned read-back of the decision
  uint32_t* h_pf_kept = nullptr;      // pinned: so_icp_transform_cloud's count of kept points
  size_t pf_temp_for = 0, pf_temp_need = 0;  // map_sort_temp_bytes(pf_temp_for) == pf_temp_need (the query costs two library calls)
  bool pf_fast = true;                // SOICP_PREFILTER_FAST=0: statistics read back, decided on the host, then the filter (rounds 1-3)
  // so_icp_set_cloud_intensity: byte offset of the FLOAT32 intensity in a point record, -1: off (the map's fourth lane stays 0)
  int intensity_off = -1;
  DevBuf d_inten;                     // so_icp_localization on a host scan: the scan's intensities next to resolve_scan's packed xyz
  float* h_inten = nullptr; size_t h_inten_cap = 0;  // pinned: where they are gathered from the caller's records
  DevBuf pf_inten;                    // the pre-filter's intensities, index for index with pf_out
  size_t pf_inten_n = 0; bool pf_inten_on = false;   // points of the last pre-filter's output / the switch was on during it
  hipEvent_t ev_upload = nullptr;     // a scan uploaded through the auxiliary queue: the context's queue waits for it
  std::shared_ptr<void> fe_state;     // so_icp_extract_features(_dev) (feature_extraction.cpp)
  std::shared_ptr<void> rs_state;     // so_icp_registered_scan(_dev) (feature_extraction.cpp): buffers of its own
  // so_icp_keep_correspondences / so_icp_correspondences (correspondences.cpp): the switch, the packed copy of the last registered
  // scan (the records themselves stay in d_nd / d_coeff / d_status), and what the last registration-family call left for the export
  bool corr_keep = false;
  DevBuf corr_scan;
  struct CorrLast {
    bool valid = false;               // the last registration-family call ended with SO_ICP_OK, with the switch on
    size_t n = 0; uint32_t n_accepted = 0;   // points of the scan / iterations[last].num_surf_from_scan
    double a2 = 0; int variant = 0;   // EvalParams::a2 / ::variant of that registration
    int outer_iteration = 0;
    double pose_fit[7] = {0, 0, 0, 0, 0, 0, 1}, pose_eval[7] = {0, 0, 0, 0, 0, 0, 1};  // where the set was formed / the default evaluation pose
    int32_t hist[16] = {};            // reject_hist[7] | obs_hist[9] of the outer iteration that formed the set (so_icp_correspondence_sums)
    // so_icp_correspondence_geometry: the call that left the set also left the neighbour snapshot; the gates of THAT registration
    bool geometry = false;
    float sq_max_dist_f = 0; double max_point_dist = 0;   // MatchParams::sq_max_dist_f / ::max_point_dist
  } corr_last;
  bool corr_geom_keep = false;        // so_icp_keep_correspondence_geometry: the switch (never on without corr_keep)
  std::shared_ptr<void> corr_geom_state;  // so_icp_correspondence_geometry: the snapshot and the export's own buffers
  std::shared_ptr<void> corr_state;   // so_icp_correspondences: buffers of its own
  std::shared_ptr<void> corr_sums_state;  // so_icp_correspondence_sums: buffers of its own
  // so_icp_keep_batch_correspondences / so_icp_keep_sequence_correspondences (selection_correspondences.cpp): the switches, and what the
  // last so_icp_register_batch / the last so_icp_register_sequence or so_icp_localization_sequence left while its switch was on -- the
  // records of ALL its entries (hypotheses / frames), entry k at element at[k] of nd / coeff / status, the packed scan of entry k at
  // point scan_at[k] of `scan`, and per entry what note_correspondences keeps of a single registration.
  //   a batch: one scan copy for all hypotheses (scan_at = 0), hypothesis h at h * bs (BatchBufs::bs of that batch): the batched kernels
  //     of the group that starts at `base` write slice base + their own index, a lane copies its context's arrays into slice h
  //   a run:   a scan copy per frame at the frame's records (scan_at = at; a slice has the padding of the context's own arrays and starts
  //     at a multiple of 64: 32 + 8 + 1 + 12 = 53 bytes per point and frame): a frame started by sequence.cpp's chained path gets its
  //     slice as the kernel arguments of its sweeps and solves, a frame that went through a per-frame entry copies the context's arrays
  //     there (seq_corr_note_plain)
  // Two independent sets -- both switches may be on --, each with export buffers of its own.  No other entry writes any of it.
  struct KeptSets {
    DevBuf nd, coeff, status, scan;
    std::vector<size_t> n, at, scan_at;  // per entry: its points, its first element, the first point of its scan
    size_t total = 0;                    // elements of nd / coeff / status
    bool valid = false;                  // the last batch with the switch on returned without an error / the last run got as far as frame 0
    std::vector<CorrLast> rec;           // per entry; valid = the hypothesis / the frame ended with SO_ICP_OK
    int entries() const { return (int)n.size(); }
    CorrBuffers slice(size_t k) const { return CorrBuffers{nd.as<double4>() + at[k], coeff.as<double>() + at[k], status.as<uint8_t>() + at[k]}; }
    float* scan_of(size_t k) const { return scan.as<float>() + 3 * scan_at[k]; }
    ~KeptSets() { for (DevBuf* b : {&nd, &coeff, &status, &scan}) b->release(); }
  };
  bool batch_corr_keep = false, seq_corr_keep = false;
  std::unique_ptr<KeptSets> batch_corr, seq_corr;
  std::shared_ptr<void> batch_corr_state, seq_corr_state;  // the exports and sums of each set: buffers of their own
  int seq_corr_frame = -1;                // >= 0: the per-frame entry in progress is this frame of a run that keeps its sets (seq_corr_note_plain)
  // so_icp_match(_dev): the registration in progress is one outer iteration's matching half and the evaluation at the guess (one
  // outer iteration, ZERO LM iterations, per-evaluation launches); it leaves tracker, staged scans and packing policy alone
  bool match_only = false;
  // The pose priors that wait for the NEXT entry of their kind (reg_plan.h: PriorKind, refused_prior) -- one slot, since the setters
  // refuse one another: at most one kind is pending.
  //   kPriorSingle (so_icp_set_pose_prior): `single`, the last argument of the solve / evaluation launches of the registration that
  //     carries it; so_icp_register(_dev) and so_icp_localization(_dev) consume it when they return (PriorOneShot)
  //   kPriorsRun (so_icp_set_sequence_priors), kPriorsBatch (so_icp_set_batch_priors): one prior and one mode (SO_ICP_PRIOR_*) per
  //     frame / per hypothesis (its guess: poses_in[k]); the sequence or batch call takes them out of the context when it starts
  //     (take), so the per-frame entries it runs do not meet them and they are consumed whatever it returns
  struct PriorSet {
    PriorKind kind = kPriorsNone;
    PosePrior single{};
    std::vector<PosePrior> priors;
    std::vector<uint8_t> modes;
    void withdraw(PriorKind k) { if (kind == k) { kind = kPriorsNone; priors.clear(); modes.clear(); } }  // (another kind stays)
    // a call of another length than the pending priors of its kind is refused and leaves them where they are
    bool count_matches(PriorKind k, int count) const { return kind != k || (size_t)count == priors.size(); }
    PriorSet take(PriorKind k) {  // -> the priors of kind k, out of the context; an empty set where none are pending
      PriorSet out;
      if (kind == k) { out.kind = k; out.priors.swap(priors); out.modes.swap(modes); kind = kPriorsNone; }
      return out;
    }
    bool any() const { for (uint8_t m : modes) if (m != SO_ICP_PRIOR_NONE) return true; return false; }
    int mode(int k) const { return (size_t)k < modes.size() ? modes[(size_t)k] : SO_ICP_PRIOR_NONE; }
    // P_k: priors[k], with T_meas = the element's guess where the mode says so; false: element k carries no prior
    bool frame_prior(int k, const double guess[7], PosePrior& out) const {
      if (mode(k) == SO_ICP_PRIOR_NONE) return false;
      out = priors[(size_t)k];
      if (mode(k) == SO_ICP_PRIOR_AT_GUESS) std::memcpy(out.T_meas, guess, sizeof(out.T_meas));
      return true;
    }
    // element k through a per-frame entry (so_icp_register(_dev), so_icp_localization(_dev), register_core on a batch lane): P_k becomes
    // the single prior of `c`, whose own priors were taken out -- what so_icp_set_pose_prior does, without its refusals
    void arm(so_icp_ctx* c, int k, const double guess[7]) const { c->pending.kind = frame_prior(k, guess, c->pending.single) ? kPriorSingle : kPriorsNone; }
  } pending;
  hipStream_t pf_stream = nullptr;   // the pre-filter's own queue: the next frame's upload + VoxelGrid run BESIDE the map insert the previous
  // Seam B scratch
  DevBuf d_q, d_nbr, d_d2, d_idx, d_found, d_fblist;
  // persistent LidarSLAM state
  int32_t prev_obs_hist[SO_ICP_N_OBS]{};
  bool have_hist = false;
  int last_pos[3] = {0, 0, 0};
  // so_icp_register_batch: worker contexts register hypotheses concurrently against the PARENT's resident map
  struct Borrow { bool on = false; DevMapView view{}; float plane_res = 0; int pos[3] = {0, 0, 0}; int count_5x5 = 0; } borrow;
  std::vector<so_icp_ctx*> workers;
  // so_icp_register_batch, batched kernels: one set of per-registration arrays per hypothesis (common element stride bs)
  struct BatchBufs {
    uint32_t cap_hyp = 0, bs = 0, table_log2 = 0;
    bool tables_clean = false;
    DevBuf states, begin, active, qslot, qrank, binned, chunks, status, nbr5, nd, coeff, bin_key, bin_cnt, bin_off, partials, sync, hist;
    DevState* h_states = nullptr; RegBeginArgs* h_begin = nullptr; uint32_t* h_active = nullptr;  // pinned
    // so_icp_set_batch_priors: the table of per-hypothesis prior blocks (kBatchPriorStride doubles each, kernels.h) and its pinned
    // source; reserved by the first batch that carries a prior, never by one that does not
    DevBuf priors; double* h_priors = nullptr; uint32_t cap_prior_hyp = 0;
    void release() {
      for (DevBuf* b : {&states, &begin, &active, &qslot, &qrank, &binned, &chunks, &status, &nbr5, &nd, &coeff, &bin_key, &bin_cnt,
                        &bin_off, &partials, &sync, &hist, &priors}) b->release();
      if (h_states) (void)hipHostFree(h_states);
      if (h_begin) (void)hipHostFree(h_begin);
      if (h_active) (void)hipHostFree(h_active);
      if (h_priors) (void)hipHostFree(h_priors);
      h_states = nullptr; h_begin = nullptr; h_active = nullptr; h_priors = nullptr; cap_hyp = 0; bs = 0; table_log2 = 0; tables_clean = false;
      cap_prior_hyp = 0;
    }
  } batch;
  int batch_degrade = 0;  // 0: two solve workgroups per compute unit, 1: one (after a batched solve that was not co-resident, or
                          // SOICP_BATCH_MODE=one_per_cu), 2: lanes = concurrent sequential registrations (SOICP_BATCH_MODE=lanes)
  bool no_map_shift_once = false;  // retry of a registration: keep the window of the first attempt
  int n_cus = 256;            // compute units of the device: upper bound of the persistent solve launch's workgroups
  int ablate = 0;             // SOICP_ABLATE (profiling / test switches), read at creation
  bool speculate = true;      // enqueue outer iteration i+1 before the report of i is in (SOICP_SPECULATE=0: wait first)
  // (round 5: no event and no stream query accompanies the host's wait for a report in the normal case.  An event record is a
  //  marker packet, and so is what hipStreamQuery enqueues to learn whether the queue has drained: either one landed between the
  //  speculated k-NN sweep and the solve launch enqueued behind it, where the command processor spent ~6 us on it -- the gap
  //  every kernel trace of rounds 3-5 shows in front of the second solve.  The watchdog of that wait is now the clock: the queue
  //  is queried only after kReportWatchdogMs without a report -- await_report, icp_context.cpp.)
  bool batch_mode = false;    // no kernel timing, tracker state read-only
  bool batch_single = false;  // batch on ONE lane: nothing runs next to it, the persistent solve launch is safe
  bool no_map_shift = false;  // so_icp_register_batch: hypotheses after the first keep the window of the first
  int startup_count = 0;
  double last_time = 0;
  // timing
  std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
  std::vector<EventSpan> spans;
  bool span_open = false;
  so_icp_timing timing{};
  // RCCL
  Rccl rccl; ncclComm_t comm = nullptr;
  std::shared_ptr<InprocGroup> group;  // so_icp_comm_init_inprocess
  // peer exchange (so_icp_peer_export / _connect / _enable): tagged-chunk push between the ranks' persistent solve launches
  void* peer_own = nullptr;                 // this rank's inbox (uncached / fine-grained device memory)
  void* peer_inbox[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  bool peer_opened[8] = {false, false, false, false, false, false, false, false};  // mapped with hipIpcOpenMemHandle (to be closed)
  bool peer_connected = false, peer_on = false;
  unsigned peer_connects = 0;  // handshakes so far (tag of the self-test chunks)
  // so_icp_stage_scan: the NEXT scans travel to HBM while the current registration runs -- straight from the caller's buffer
  // when that is registered (pinned) host memory (so_icp_host_register: the announcing thread enqueues the DMA on the copy
  // stream and returns; the registration's first kernel waits for it ON THE DEVICE), else through a copy thread that packs
  // the cloud into a pinned buffer first.
  static constexpr int kStageSlots = 3;  // one in use by the registration in flight + two announced ahead
  struct StageSlot {
    const float* src = nullptr; size_t n = 0, stride = 0;  // identity of the staged host buffer
    DevBuf dev; float* pinned = nullptr; size_t pinned_cap = 0;
    StageState state = StageState::kEmpty;
    unsigned long long seq = 0;          // announcement number (newer scans have larger ones)
    hipEvent_t ev = nullptr;             // direct path: end of the H2D copy on the copy stream
    bool ev_pending = false;             //   ... which may still be reading the caller's buffer
    bool deferred = false;               // direct path: announced, the copy is not enqueued yet (see stage_issue_deferred)
    hipStream_t tail_stream = nullptr;   // direct path: the copy is enqueued there, what follows it (binning ahead, `ev`) not yet -- see stage_tail
    std::chrono::steady_clock::time_point t_announced;
    std::string err;
    // binned ahead (stage_prebin): the scan's work list, built on the copy queue behind the copy while the registration before it runs
    DevBuf pb_keys, pb_vals, pb_chunks, pb_binned, pb_ctr;
    bool prebinned = false; uint32_t pb_chunk_cap = 0;
    hipError_t reserve_worklist(size_t n) {  // the pb_* buffers for a scan of n points
      const size_t m = n + 256;
      hipError_t e = pb_keys.reserve(m * 4);
      if (e == hipSuccess) e = pb_vals.reserve(m * 4);
      if (e == hipSuccess) e = pb_chunks.reserve(m * 4);
      if (e == hipSuccess) e = pb_binned.reserve(m * 16);
      if (e == hipSuccess) e = pb_ctr.reserve(64);
      return e;
    }
    void release() {
      for (DevBuf* b : {&dev, &pb_keys, &pb_vals, &pb_chunks, &pb_binned, &pb_ctr}) b->release();
      if (pinned) (void)hipHostFree(pinned);
      if (ev) (void)hipEventDestroy(ev);
    }
  } stage[kStageSlots];
  // Binning ahead (round 5).  A scan announced with so_icp_stage_scan is hash-binned on the copy queue right behind its DMA, under the
  // guess of the registration that enqueues the copy (the latest pose this context knows), so that its own registration starts
  // with the k-NN sweep: scan_keys -> bin_offsets -> bin_place (three dependent launches, ~21 us of a 150 us registration) leave
  // the registration's critical path and run beside the previous registration's solve, which keeps one wavefront per SIMD busy.
  // Chunks binned under a pose one frame old stay spatially compact under the scan's own guess -- the k-NN kernel forms every
  // chunk's candidate block from the queries' actual positions, as it does for the second sweep of any registration; results
  // do not depend on the binning (exact per query, sums in scan order).  Single device, device-resident map only; SOICP_PREBIN=0
  // switches it off.
  bool prebin = true;
  BinHashTable pbin;
  StageSlot* stage_in_use = nullptr;  // the slot the current registration reads (released when the call returns)
  unsigned long long stage_seq = 0, stage_consumed_seq = 0;  // announcements so far / announcement number of the scan consumed last
  bool stage_quit = false, stage_started = false;
  std::atomic<int> stage_pending{0};      // queued slots the copy thread has not picked up yet
  std::atomic<bool> stage_parked{false};  // the copy thread sleeps on stage_cv (it spins for a while after every job first)
  std::atomic<bool> stage_timed{false};   // ... in the TIMED wait for a DMA-staged scan's 300 us: it looks at the slots again by itself when that
                                          // runs out, so another DMA announcement need not wake it (a futex call on the announcing thread's path)
  std::thread stage_thread; std::mutex stage_mu; std::condition_variable stage_cv;
  struct HostRange { const char* p; size_t bytes; bool owned; };
  std::vector<HostRange> host_ranges;     // so_icp_host_register / so_icp_host_alloc (under stage_mu)
  // so_icp_register_sequence: a copy / binning queue and three scan slots of its own (nothing shared with so_icp_stage_scan's
  // slots and thread), the iterations pre-enqueued per registration, DevState::done_count as of the last report
  hipStream_t seq_stream = nullptr;
  StageSlot seq_slot[kStageSlots];
  BinHashTable sbin;
  int seq_depth = 2; uint32_t done_count_seen = 0;
  // so_icp_sequence_announce_next: the scan that will START the next so_icp_register_sequence call -- copied and binned beside the LAST
  // registration of the current call (under that registration's guess o delta), adopted by the next call when its scans[0] is this buffer
  struct SeqNext { const void* next_scan = nullptr; size_t next_n = 0; double delta[7] = {0, 0, 0, 0, 0, 0, 1}; bool announced = false;  // for the coming call to stage
                   const void* scan = nullptr; size_t n = 0;                                                                             // staged by the last call
                   bool staged = false; int slot = 0; bool binned = false, needs_event = false; const float* d_scan = nullptr; } seq_next;
  bool seq_chain = true;                  // SOICP_SEQ_CHAIN=0: so_icp_register_sequence runs one registration after the other (same results)
  bool query_waves = true;                // SOICP_QUERY_WAVES=0: a small scan (<= 4 096 kept queries) is binned and swept in chunks like a large one
  bool knn_pack = true;                   // SOICP_KNN_PACK=0: one chunk per wavefront throughout (round-3 work list)
  bool knn_list_fits = false;             // the last registration's work list (normal + light chunks) fitted the k-NN grid one chunk per wavefront:
                                          // packing four light chunks into a wavefront then only lengthens the longest wavefronts (a 13 k-point
                                          // voxel-filtered scan: sweeps 20.5 + 18.6 -> 17.2 + 16.9 us unpacked)
  uint32_t packed_leftover_seen = 0;      // DevState::packed_leftover (a running count) as of the last report
  int knn_pack_hold = 0;                  // registrations left without packing after one in which the packed near pass left > 3 % of
                                          // the queries to the exact per-lane scan (sparse map, far-off guess): then it is not a saving
  static constexpr int kBatchRoundsTracked = 16;
  float batch_survivors[kBatchRoundsTracked] = {};  // so_icp_register_batch: share of round r's list still active after it, last batch (chaining of rounds)
  bool batch_chain = true;                // (SOICP_BATCH_CHAIN=0: report + synchronisation after every round, as in round 3)
  hipStream_t copy_stream = nullptr;
  bool retried = false;       // the current registration is the repeat of an abandoned one
  unsigned long long peer_timeout_ticks = 100000000ull;  // 1 s at 100 MHz: patience of a solve launch with the peer exchange (SOICP_PEER_TIMEOUT_MS)
  bool scan_staged = false;   // the scan of the current registration came from a stage slot
  bool query_split = false;   // world_size > 1, SO_ICP_SHARD_QUERIES: map replicated, the scan's 64-point segments dealt to the ranks
  DevBuf d_sub;               //   this rank's share of the current scan, gathered

  ~so_icp_ctx();
};

#define HIP_TRY(ctx, expr)                                                                         \
  do {                                                                                             \
    hipError_t e__ = (expr);                                                                       \
    if (e__ != hipSuccess) {                                                                       \
      (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e__);                             \
      return SO_ICP_E_HIP;                                                                         \
    }                                                                                              \
  } while (0)

namespace soicp::host {

// sets the text so_icp_last_error returns and passes `code` through
inline int fail(so_icp_ctx* c, int code, const std::string& msg) { c->err = msg; return code; }
using PriorSet = so_icp_ctx::PriorSet;
// so_icp_set_pose_prior: so_icp_register(_dev) and so_icp_localization(_dev) consume the pending single prior when they return, whatever
// they return
struct PriorOneShot { so_icp_ctx* c; ~PriorOneShot() { c->pending.withdraw(kPriorSingle); } };
// An entry that takes priors of kind `accepted` (kPriorsNone: none) is refused while another kind is pending, which stays (refused_prior)
inline int refuse_pending(so_icp_ctx* c, const char* entry, PriorKind accepted) {
  switch (refused_prior(c->pending.kind, accepted)) {
    case kPriorSingle:
      return fail(c, SO_ICP_E_UNSUPPORTED, std::string(entry) + ": a pose prior is pending (so_icp_set_pose_prior); it goes into so_icp_register(_dev) "
                                           "or so_icp_localization(_dev) -- withdraw it with so_icp_set_pose_prior(ctx, NULL) first");
    case kPriorsRun:
      return fail(c, SO_ICP_E_UNSUPPORTED, std::string(entry) + ": the priors of a run are pending (so_icp_set_sequence_priors); they go into "
                                           "so_icp_register_sequence or so_icp_localization_sequence -- withdraw them with "
                                           "so_icp_set_sequence_priors(ctx, 0, NULL, NULL) first");
    case kPriorsBatch:
      return fail(c, SO_ICP_E_UNSUPPORTED, std::string(entry) + ": the priors of a batch are pending (so_icp_set_batch_priors); they go into "
                                           "so_icp_register_batch -- withdraw them with so_icp_set_batch_priors(ctx, 0, NULL, NULL) first");
    case kPriorsNone: break;
  }
  return SO_ICP_OK;
}
// what a DeviceMap member returns (device_map.h: -1 out of memory / a full cube, -2 a HIP error, its text in c->err; else >= 0) as a C ABI code
inline int map_status(int r) { return r >= 0 ? SO_ICP_OK : (r == -1 ? SO_ICP_E_NOMEM : SO_ICP_E_HIP); }
// the stride rule of the entries that read float x y z records: 0 means packed (12 bytes); a multiple of 4
// where record i's intensity is, given where its x is: inside the record when the switch is on and the record holds it, else nowhere (0)
inline const float* intensity_in(const so_icp_ctx* c, const float* xyz, size_t stride_bytes) {
  return (c->intensity_off >= 0 && stride_bytes >= (size_t)c->intensity_off + 4) ? xyz + c->intensity_off / 4 : nullptr;
}
inline int normalise_stride(so_icp_ctx* c, size_t* stride_bytes) {
  if (*stride_bytes == 0) *stride_bytes = 12;
  return *stride_bytes % 4 ? fail(c, SO_ICP_E_INVALID, "stride_bytes must be a multiple of 4") : SO_ICP_OK;
}

}  // namespace soicp::host

#define NEED_DEVICE(c)                                                                                        \
  do {                                                                                                        \
    if ((c)->host_only)                                                                                       \
      return fail((c), SO_ICP_E_HIP, "host-only context (device_id < 0): no compute path -- libsoicp has no CPU fallback"); \
  } while (0)

// ---- helpers that more than one translation unit calls ---------------------------------------------------------------------
namespace soicp::host {

extern thread_local std::string g_create_error;  // so_icp_last_error(NULL): the last failed so_icp_create / so_icp_comm_unique_id

// icp_context.cpp
hipEvent_t next_event(so_icp_ctx* c);  // a timing event of the context's pool
float map_plane_res(const so_icp_ctx* c);
void map_shift(so_icp_ctx* c, const double t[3], int pos[3]);
int map_count_5x5(const so_icp_ctx* c, const int pos[3]);
const int* map_origin(const so_icp_ctx* c);
int upload_map(so_icp_ctx* c);
int reserve_scan_buffers(so_icp_ctx* c, size_t n);
MatchParams match_params(float plane_res, int ablate);
EvalParams eval_params(float plane_res, int variant, int ablate);
unsigned long long registration_params(so_icp_ctx* c, float plane_res, size_t n, uint32_t chunk_cap, int ring, MatchParams& mp, EvalParams& ep);
int refuse_scan_size(so_icp_ctx* c);  // a scan of kMaxScanPoints or more: SO_ICP_E_UNSUPPORTED with its text
// What the sweep and solve launches of one registration read: the scan, its work list, the correspondences, the loop bounds
// (so_icp_register's RegPlan and so_icp_register_sequence's SeqRun are both one of these and more)
struct RegWork {
  const float* d_scan = nullptr; size_t n = 0;
  bool query_waves = false;                                             // every kept query a wavefront of its own: no work list
  const float4* d_binned = nullptr; const uint32_t* d_chunks = nullptr;  // the work list of a scan swept in chunks
  CorrBuffers corr{nullptr, nullptr, nullptr};
  int max_outer = 0, lm_max = 0;
};
// One k-NN sweep.  `mp_it`: the caller's copy of the registration's parameters for this sweep (publish_prev is the caller's policy);
// `first`: outer iteration 0; `begin_slot`: the registration's prologue rides on this sweep of a scan binned ahead (MatchParams::begin),
// its counters are in that slot; `pose`, `chain_expect`: the prologue's guess / the chained start's condition
void launch_sweep(so_icp_ctx* c, const RegWork& w, MatchParams& mp_it, bool first, const so_icp_ctx::StageSlot* begin_slot, const double pose[7],
                  uint32_t chain_expect, hipEvent_t ev_start, hipEvent_t ev_stop);
// The whole solve of one outer iteration in one launch; gives `ep_it` (the caller's copy: defer_publish, chain_*) its epoch
// (`prior`: the registration's pose prior; `prior_at_guess`: its T_meas is the guess on the device, launch_solve)
void launch_persistent_solve(so_icp_ctx* c, const RegWork& w, EvalParams& ep_it, const MatchParams& mp, const PosePrior* prior = nullptr,
                             bool prior_at_guess = false);
// The host's wait for the report `want` in a pinned mirror's seq word; `s`: the queue whose draining ends the wait without one.  The
// mirrors are polled; the watchdog of that wait is the clock and, once it has run out, the queue (so_icp_ctx::speculate has the
// measured reason why nothing -- no event, no stream query -- accompanies the wait in the normal case).
enum class Report { kReported, kDrained /* every launch completed, no report */, kHipError /* c->err is set */ };
Report await_report(so_icp_ctx* c, const volatile unsigned long long* seq, unsigned long long want, hipStream_t s);
// the head of so_icp_stats every registration entry fills alike: uncertainty, window position, map and scan counts, startup_count
void fill_stats_header(const so_icp_ctx* c, so_icp_stats* st, const int pos[3], int count_5x5, size_t n);
// what a finished registration, reported in `mirror`, leaves in the context: h_state, the packing policy, knn_list_fits, done_count_seen
void note_registration_done(so_icp_ctx* c, DevState* mirror, const MatchParams& mp, size_t n, bool sets_list_fits, bool sets_done_count);
void fill_result(so_icp_ctx* c, const DevState& H, const double pose_in[7], so_icp_stats* st, double pose_out[7], bool update_tracker);
constexpr int kRetryWithoutPersistentSolve = -1000;  // internal: never leaves register_core
int register_core(so_icp_ctx* c, const float* d_scan, size_t n, const double pose_in[7], double pose_out[7], so_icp_stats* st);
hipStream_t aux_stream(so_icp_ctx* c);
int upload_scan_impl(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, DevBuf& dst, bool wait = true);

// staging.cpp
void stage_issue_deferred(so_icp_ctx* c, const double* prebin_pose);
void stage_issue_deferred_copy(so_icp_ctx* c);
int resolve_scan(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, const float** d_scan);
void drop_staged(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes);
void release_staged(so_icp_ctx* c);
bool bin_into_slot(so_icp_ctx* c, const float* d_scan, size_t n, const double pose[7], hipStream_t s, BinHashTable& table,
                   so_icp_ctx::StageSlot& sl);

// correspondences.cpp: what the registration entries do for so_icp_correspondences while so_icp_ctx::corr_keep is on
inline bool keeps_correspondences(const so_icp_ctx* c) { return c->corr_keep && !c->batch_mode && !c->borrow.on && c->cfg.world_size <= 1; }
int keep_scan_copy(so_icp_ctx* c, const float* d_scan, size_t n);  // the packed copy, enqueued on the context's queue
// the record of a registration that ended with SO_ICP_OK, reported in H from the guess `guess` with the loss parameters of `ep`
void note_correspondences(so_icp_ctx* c, const DevState& H, const double guess[7], size_t n, const EvalParams& ep);
// the same record into `L` (so_icp_keep_batch_correspondences: one per hypothesis)
void fill_correspondence_record(so_icp_ctx::CorrLast& L, const DevState& H, const double guess[7], size_t n, const EvalParams& ep);
// selection_correspondences.cpp: what so_icp_register_batch does while so_icp_ctx::batch_corr_keep is on.  The set of a batch of n_hyp
// hypotheses of n points: arrays at stride `bs` reserved, every record invalid, the packed scan copy enqueued on the context's queue
int batch_corr_begin(so_icp_ctx* c, const float* d_scan, size_t n, int n_hyp, uint32_t bs);
// what the two sequence entries do while so_icp_ctx::seq_corr_keep is on.
inline bool keeps_sequence_correspondences(const so_icp_ctx* c) { return c->seq_corr_keep && c->cfg.world_size <= 1; }
// The set of a run of `count` frames of n_points[k] points: every array reserved for the sum of the frames (SO_ICP_E_NOMEM when that
// cannot be had), every record invalid.  Before the run's first launch; nothing of the set is allocated after it
int seq_corr_begin(so_icp_ctx* c, int count, const size_t* n_points);
// frame k's packed scan copy, device to device on queue `s`
int seq_corr_copy_scan(so_icp_ctx* c, int k, const float* d_scan, hipStream_t s);
// the context's own d_nd / d_coeff / d_status into frame k's slice, three copies on the context's queue (as a batch lane does)
int seq_corr_copy_records(so_icp_ctx* c, int k);
// frame k ended with SO_ICP_OK, reported in H from `guess` with the loss of `ep`: its host record
void seq_corr_note(so_icp_ctx* c, int k, const DevState& H, const double guess[7], const EvalParams& ep);
// register_core, for a frame that goes through a per-frame entry (so_icp_ctx::seq_corr_frame >= 0): scan copy, record copies and the
// host record, behind the registration's report and in front of whatever the entry enqueues next (so_icp_localization: the insert)
int seq_corr_note_plain(so_icp_ctx* c, const float* d_scan, size_t n, const DevState& H, const double guess[7], const EvalParams& ep);
// a run that returned an error leaves no frame's set
void seq_corr_fail(so_icp_ctx* c);
// so_icp_keep_correspondence_geometry: what the same entries do for so_icp_correspondence_geometry while so_icp_ctx::corr_geom_keep is on
inline bool keeps_correspondence_geometry(const so_icp_ctx* c) { return c->corr_geom_keep && keeps_correspondences(c); }
// the snapshot of the n points' status bytes, neighbour indices and neighbour points: one launch on the context's queue, behind the
// launch that produced the final report and in front of whatever changes the map next (reads d_status, d_nbr5 and c->view)
int keep_neighbour_snapshot(so_icp_ctx* c, size_t n);
// behind note_correspondences: the kept set has its snapshot, taken under the gates of `mp`
void note_correspondence_geometry(so_icp_ctx* c, const MatchParams& mp);

// multi_gpu.cpp
int exchange_map_counts(so_icp_ctx* c);
int reshard_for_resolution(so_icp_ctx* c, float line_res, float plane_res);
bool group_allreduce(so_icp_ctx* c, LmSums* io);
void group_abort(so_icp_ctx* c);
void group_leave(so_icp_ctx* c);

}  // namespace soicp::host
