// reg_plan.h -- the decisions of a registration's host schedule that need no device: limits, the query split, table and work-list
// sizes, the window rule of a chained start.  Plain arithmetic, one definition each for icp_context.cpp, sequence.cpp, batch.cpp and
// staging.cpp; compiled for the host alone by tests/native/reg_plan_host.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "so_math.h"

namespace soicp::host {

// loop bounds of a registration: LidarSlam.h:273 (4 outer iterations, 4 LM iterations where the configuration gives none); the
// caps are the per-iteration statistics of so_icp_stats (SO_ICP_MAX_OUTER, checked in ctx.h) and the solve launch's slots
constexpr int kOuterCap = 16, kLmCap = 16;
inline int outer_limit(int max_iterations) { return std::min(max_iterations > 0 ? max_iterations : 4, kOuterCap); }
inline int lm_limit(int lm_max_iterations) { return std::min(lm_max_iterations > 0 ? lm_max_iterations : 4, kLmCap); }

// Pose priors wait in ONE slot of the context for the entry that takes their kind: a single prior for so_icp_register(_dev) /
// so_icp_localization(_dev), the priors of a run for the two sequence entries, the priors of a batch for so_icp_register_batch.  An entry
// (a setter included) that takes kind `accepted` -- kPriorsNone: so_icp_match(_dev), which takes none -- goes on when the slot is empty
// or holds that kind; otherwise it is refused because of what is pending, and that stays.  -> kPriorsNone: go on; else the kind in the way
enum PriorKind { kPriorsNone = 0, kPriorSingle = 1, kPriorsRun = 2, kPriorsBatch = 3 };
inline PriorKind refused_prior(PriorKind pending, PriorKind accepted) { return pending == accepted ? kPriorsNone : pending; }

// so_icp_set_pose_prior: the pending prior (`pending`: the slot holds a single prior) goes into a registration that is the context's own
// (no batch lane, no borrowed map), on one device, and a registration (so_icp_match refuses it)
inline bool carries_pose_prior(bool pending, bool own, int world_size, bool match_only) { return pending && own && world_size <= 1 && !match_only; }

// so_icp_set_sequence_priors: which persistent-solve kernel the launches of frame k of so_icp_register_sequence's chained path use.
// `mode`: the frame's SO_ICP_PRIOR_* (0 none, 1 given, 2 at the guess); `chained`: the frame's BEGIN launch takes its guess from
// DevState::T_chain, so the host holds only a prediction of it.  Wherever the host knows the guess exactly -- frame 0, an unchained
// start, the start after a broken chain -- it fills T_meas itself and solve_kernel_prior serves both modes.
enum SolveKernelKind { kSolvePlain = 0, kSolvePrior = 1, kSolvePriorAtGuess = 2 };
inline SolveKernelKind sequence_solve_kernel(int mode, bool chained) {
  return mode == 0 ? kSolvePlain : ((mode == 2 && chained) ? kSolvePriorAtGuess : kSolvePrior);
}
// so_icp_set_batch_priors: which batched solve kernel a round of so_icp_register_batch launches for the hypotheses active[0 .. n_active)
// of its group.  `modes`: SO_ICP_PRIOR_* per hypothesis of the group (nullptr: the batch carries no priors).  The kernel with the prior
// table only where a hypothesis of the list carries a prior; every other round launches what a batch without priors launches.
enum BatchSolveKernelKind { kBatchSolvePlain = 0, kBatchSolvePrior = 1 };
inline BatchSolveKernelKind batch_solve_kernel(const uint8_t* modes, const uint32_t* active, uint32_t n_active) {
  if (!modes) return kBatchSolvePlain;
  for (uint32_t k = 0; k < n_active; ++k)
    if (modes[active[k]] != 0) return kBatchSolvePrior;
  return kBatchSolvePlain;
}

// so_icp_match_batch: the one launch that fits and evaluates every (hypothesis, query) of a group (match_batch_kernel) has n_act * V
// workgroups, V the grid a single registration of the same scan launches for its fit pass.  Workgroup b serves virtual workgroup b % V of
// the hypothesis active[b / V] -- the workgroups of a hypothesis are consecutive, so they are dispatched together.  constexpr: the
// kernel calls these too
struct MatchBatchSlot { uint32_t entry, vb; };  // entry: index into the launch's active list
constexpr MatchBatchSlot match_batch_slot(uint32_t b, uint32_t V) { return MatchBatchSlot{b / V, b - (b / V) * V}; }
// Where hypothesis h keeps the workgroup records of that launch and counts their arrivals: inside ITS share of the batch's record table
// (partial_stride doubles per hypothesis, BatchView) and of the hand-off block (sync_stride words per hypothesis).  The record table is
// the batched solve's, 16-byte chunks {value, pass tag | counter}: the match writes value a of virtual workgroup vb into the VALUE half of
// chunk a * max_grid + vb and never a tag, so a solve launch behind it on the same context finds no chunk that claims to be of its pass.
// The arrival counter is word 0 of the hypothesis' hand-off block (the first arrival counter; the batched solve uses none of them).
constexpr size_t match_batch_partial_word(size_t h, uint32_t partial_stride, uint32_t a, uint32_t vb, uint32_t max_grid) {
  return h * partial_stride + 2u * ((size_t)a * max_grid + vb);
}
constexpr size_t match_batch_ticket_word(size_t h, uint32_t sync_stride) { return h * sync_stride; }

// so_icp_batch_correspondences: the layout of one export over a selection of the last batch's hypotheses.
// Entry k of the selection is hypothesis hyp[k] (hyp == nullptr: k).  -> the first entry whose index lies outside [0, n_hyp), -1: none
inline int batch_selection_first_bad(const int32_t* hyp, int n_sel, int n_hyp) {
  for (int k = 0; k < n_sel; ++k) {
    const int h = hyp ? hyp[k] : k;
    if (h < 0 || h >= n_hyp) return k;
  }
  return -1;
}
// The records of entry k occupy [first_record[k], first_record[k + 1]): as wide as the count its hypothesis reported, 0 for a hypothesis
// that left no set; an index that repeats gets a range of its own each time.  `accepted`, `valid`: per hypothesis of the batch.
// -> first_record[n_sel], the records of the whole selection
inline uint64_t batch_record_ranges(const uint32_t* accepted, const uint8_t* valid, const int32_t* hyp, int n_sel, uint64_t* first_record) {
  uint64_t at = 0;
  for (int k = 0; k < n_sel; ++k) {
    const int h = hyp ? hyp[k] : k;
    first_record[k] = at;
    at += valid[h] ? accepted[h] : 0u;
  }
  first_record[n_sel] = at;
  return at;
}

// The same exports over a selection of a run's FRAMES (so_icp_sequence_correspondences) share all of the above; the kernels are the same
// too.  The entries' point counts -- and so their tile counts -- may differ, and an entry may have no tile at all (an empty scan, an
// entry without a set).  tile_first[0 .. n_sel]: the prefix sums of the entries' tile counts (tile_first[0] = 0, tile_first[n_sel] = the
// tickets of the launch), from the entries' points (0 for an entry without a set) and the points of a tile.  -> tile_first[n_sel]
inline uint32_t selection_tile_table(const uint32_t* n_points, uint32_t n_sel, uint32_t tile, uint32_t* tile_first) {
  uint32_t tiles = 0;
  for (uint32_t k = 0; k < n_sel; ++k) { tile_first[k] = tiles; tiles += n_points[k] / tile + (n_points[k] % tile ? 1u : 0u); }
  tile_first[n_sel] = tiles;
  return tiles;
}
// The export's workgroups draw one global ticket each.  Ticket t, 0 <= t < tile_first[n_sel], is tile t - tile_first[e] of the entry e
// with tile_first[e] <= t < tile_first[e + 1]: entry-major, so the look-back of an entry only ever waits for smaller tickets, and an
// entry without tiles gets no ticket; for entries of nblk tiles each, tile t % nblk of entry t / nblk.  n_tiles = tile_first[n_sel].
// The first look is at the entry t would belong to if all entries were equal -- a batch, a run of equal frames: found at once, the two
// words read side by side --, then a search of what is left of the prefix table (<= 11 steps for 1 024 entries).  (t x n_sel < 2^31:
// at most 2^11 tiles per entry, kMaxScanPoints, and 2^10 entries.)  constexpr: selection_correspondences_kernel calls it too
struct BatchTicket { uint32_t entry, tile; };
constexpr BatchTicket selection_ticket(uint32_t t, const uint32_t* tile_first, uint32_t n_sel, uint32_t n_tiles) {
  uint32_t lo = 0, hi = n_sel;  // tile_first[lo] <= t < tile_first[hi]
  const uint32_t guess = t * n_sel / n_tiles, first = tile_first[guess], next = tile_first[guess + 1u];
  if (first <= t) { lo = guess; if (t < next) hi = guess + 1u; } else hi = guess;
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (tile_first[mid] <= t) lo = mid; else hi = mid;
  }
  return BatchTicket{lo, t - tile_first[lo]};
}
// The status row of entry k starts at first_status[k] and is as long as its frame (valid or not): frames differ in n_points.
// -> first_status[n_sel], the bytes of all rows
inline uint64_t sequence_status_ranges(const size_t* n_points, const int32_t* frames, int n_sel, uint64_t* first_status) {
  uint64_t at = 0;
  for (int k = 0; k < n_sel; ++k) { first_status[k] = at; at += n_points[frames ? frames[k] : k]; }
  first_status[n_sel] = at;
  return at;
}

// scans of this many points or more are refused (refuse_scan_size, icp_context.cpp): the work-list counters hold 21 bits each
constexpr size_t kMaxScanPoints = (size_t)1 << 21;

// upper bound of the queries the sampling rule keeps of n points (the rule keeps ~ rate * n points)
inline size_t kept_upper_bound(int max_sf, size_t n) { return (max_sf >= 0 && n > (size_t)max_sf) ? (size_t)max_sf + 2 : n; }
// A SMALL scan -- the stock operating point of the node: max_surface_features 2000 / 4000 of a pre-filtered cloud -- is not binned at
// all: every kept query gets a wavefront of its own (knn_query_wave_kernel, up to `max_kept` = kQueryWaveMaxKept of them)
inline bool query_wave_count_ok(int max_sf, size_t n, size_t max_kept) { return n != 0 && kept_upper_bound(max_sf, n) <= max_kept; }

// SO_ICP_SHARD_QUERIES: rank's share of a scan of n points -- the 64-point segments rank, rank + world, ...; the partial last
// segment is segment number n / 64
struct QueryShare { size_t own_full; bool own_tail; size_t n_own; };
inline QueryShare query_split_share(size_t n, size_t world, size_t rank) {
  const size_t s_full = n / 64, tail = n % 64, own_full = s_full > rank ? (s_full - rank + world - 1) / world : 0;
  const bool own_tail = tail != 0 && (s_full % world) == rank;
  return QueryShare{own_full, own_tail, own_full * 64 + (own_tail ? tail : 0)};
}

// the hash table for the binning of a scan of n points: >= 2 slots per query
inline uint32_t bin_table_log2(size_t n) {
  uint32_t lg = 16;
  while ((1ull << lg) < 2 * (unsigned long long)n) ++lg;
  return lg;
}

// DevState::bin_packed = kept queries | normal chunks << 21 | light chunks << 42: the work list (normal + light chunks) fits the
// k-NN grid of `wavefronts` one chunk per wavefront
inline bool work_list_fits(unsigned long long bin_packed, unsigned long long wavefronts) { return ((bin_packed >> 21) & 0x1FFFFFull) + (bin_packed >> 42) <= wavefronts; }
inline uint32_t work_list_kept(unsigned long long bin_packed) { return (uint32_t)(bin_packed & 0x1FFFFFull); }

// The window would not roll for a pose at t (LocalMap.h:169-287: the sensor's block stays >= 3 blocks from the border), and no
// pose within `margin` of it lies in another block: placing the window for a PREDICTED guess is placing it for the actual one
inline bool cube_stable(const int origin[3], const int dims[3], const double t[3], double margin) {
  for (int a = 0; a < 3; ++a) {
    const int lo = cube_coord(t[a] - margin, origin[a]), hi = cube_coord(t[a] + margin, origin[a]);
    if (lo != hi || lo < 3 || lo >= dims[a] - 3) return false;
  }
  return true;
}
// The pose under which the scan BEHIND registration k is binned ahead and its window placed while k still runs (so_icp_register_sequence):
// k's exact guess -- known to the host since k - 1 was collected -- moved on by the next delta.  It misses the guess the device will
// form by the correction registration k makes, one frame's worth.  (Composed from the PREDICTION of k's guess instead, the corrections
// of all frames since the chain began add up: metres and tens of degrees after a few hundred frames.)
inline void predicted_guess(const double exact_guess_k[7], const double delta_next[7], double pred[7]) { pose_compose(exact_guess_k, delta_next, pred); }

}  // namespace soicp::host
