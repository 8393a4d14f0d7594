// selection_correspondences.cpp -- the correspondence sets of ALL entries of a call that registers many scans or poses, read where the call
// left them, for a selection of its entries at once:
//   so_icp_keep_batch_correspondences, so_icp_batch_correspondences, so_icp_batch_correspondence_sums           the hypotheses of
//     so_icp_register_batch.  While the switch is on a batch writes the records of all its hypotheses into arrays the context owns
//     (batch.cpp: the groups' kernels get those arrays as arguments, a lane copies its context's) and keeps ONE packed copy of the scan
//   so_icp_keep_sequence_correspondences, so_icp_sequence_correspondences, so_icp_sequence_correspondence_sums  the frames of a run
//     (so_icp_register_sequence, so_icp_localization_sequence).  While the switch is on a run writes every frame's records into a slice of
//     arrays the context owns (sequence.cpp: a frame started by the chained path gets its slice as kernel arguments; a frame that goes
//     through a per-frame entry copies the context's arrays, seq_corr_note_plain) and keeps a packed copy of every scan
// Either way the set is a so_icp_ctx::KeptSets with one small host record per entry, and there is one host path for both: the export is
// one launch of corr_kernels.hip's selection_correspondences_kernel for the whole selection, the sums two launches of
// corr_sums_kernels.hip's selection kernels -- the single exports' text, entry by entry, over entries that may differ in size.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "corr_kernels.h"
#include "ctx.h"

namespace soicp::host {

namespace {
so_icp_ctx::KeptSets& fresh_set(std::unique_ptr<so_icp_ctx::KeptSets>& slot, size_t entries) {
  if (!slot) slot = std::make_unique<so_icp_ctx::KeptSets>();
  so_icp_ctx::KeptSets& K = *slot;
  K.valid = false; K.total = 0;
  K.n.assign(entries, 0); K.at.assign(entries, 0); K.scan_at.assign(entries, 0);
  K.rec.assign(entries, so_icp_ctx::CorrLast{});
  return K;
}
}  // namespace

int batch_corr_begin(so_icp_ctx* c, const float* d_scan, size_t n, int n_hyp, uint32_t bs) {
  so_icp_ctx::KeptSets& K = fresh_set(c->batch_corr, (size_t)n_hyp);
  if (!n_hyp) { K.valid = true; return SO_ICP_OK; }  // (a batch of no hypotheses: a set nothing can be selected from)
  for (int h = 0; h < n_hyp; ++h) { K.n[(size_t)h] = n; K.at[(size_t)h] = (size_t)h * bs; }  // (one scan for all: scan_at stays 0)
  K.total = (size_t)n_hyp * bs;
  HIP_TRY(c, K.nd.reserve(K.total * sizeof(double4)));
  HIP_TRY(c, K.coeff.reserve(K.total * sizeof(double)));
  HIP_TRY(c, K.status.reserve(K.total));
  if (n) {
    HIP_TRY(c, K.scan.reserve(n * 12 + 64));
    HIP_TRY(c, hipMemcpyAsync(K.scan.p, d_scan, n * 12, hipMemcpyDeviceToDevice, c->stream));
  }
  return SO_ICP_OK;
}

int seq_corr_begin(so_icp_ctx* c, int count, const size_t* n_points) {
  so_icp_ctx::KeptSets& K = fresh_set(c->seq_corr, (size_t)count);
  auto no_set = [&] { K.n.clear(); K.at.clear(); K.scan_at.clear(); K.rec.clear(); K.total = 0; };
  size_t at = 0;
  for (int k = 0; k < count; ++k) {
    if (n_points[k] >= kMaxScanPoints) { no_set(); return SO_ICP_OK; }  // (the run refuses it: no set)
    K.n[(size_t)k] = n_points[k];
    K.at[(size_t)k] = K.scan_at[(size_t)k] = at;  // (a scan per frame, beside its records)
    at += (n_points[k] + 256 + 63) & ~(size_t)63;  // (reserve_scan_buffers' padding: a slice is as large as the array it stands for)
  }
  K.total = at;
  if (at) {
    const bool ok = K.nd.reserve(at * sizeof(double4)) == hipSuccess && K.coeff.reserve(at * sizeof(double)) == hipSuccess &&
                    K.status.reserve(at) == hipSuccess && K.scan.reserve(at * 12 + 64) == hipSuccess;
    if (!ok) {
      (void)hipGetLastError();
      no_set();
      return fail(c, SO_ICP_E_NOMEM, "so_icp_keep_sequence_correspondences: no device memory for the sets of this run (53 bytes per point and frame)");
    }
  }
  K.valid = true;
  return SO_ICP_OK;
}

int seq_corr_copy_scan(so_icp_ctx* c, int k, const float* d_scan, hipStream_t s) {
  const so_icp_ctx::KeptSets& K = *c->seq_corr;
  if (!K.valid || !K.n[(size_t)k] || !d_scan) return SO_ICP_OK;
  HIP_TRY(c, hipMemcpyAsync(K.scan_of((size_t)k), d_scan, K.n[(size_t)k] * 12, hipMemcpyDeviceToDevice, s));
  return SO_ICP_OK;
}

int seq_corr_copy_records(so_icp_ctx* c, int k) {
  const so_icp_ctx::KeptSets& K = *c->seq_corr;
  const size_t n = K.n[(size_t)k];
  if (!K.valid || !n) return SO_ICP_OK;
  const CorrBuffers to = K.slice((size_t)k);
  HIP_TRY(c, hipMemcpyAsync(to.nd, c->d_nd.p, n * sizeof(double4), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(to.coeff, c->d_coeff.p, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(to.status, c->d_status.p, n, hipMemcpyDeviceToDevice, c->stream));
  return SO_ICP_OK;
}

void seq_corr_note(so_icp_ctx* c, int k, const DevState& H, const double guess[7], const EvalParams& ep) {
  so_icp_ctx::KeptSets& K = *c->seq_corr;
  if (K.valid) fill_correspondence_record(K.rec[(size_t)k], H, guess, K.n[(size_t)k], ep);
}

int seq_corr_note_plain(so_icp_ctx* c, const float* d_scan, size_t n, const DevState& H, const double guess[7], const EvalParams& ep) {
  const int k = c->seq_corr_frame;
  if (!c->seq_corr || !c->seq_corr->valid || k < 0 || k >= c->seq_corr->entries() || c->seq_corr->n[(size_t)k] != n) return SO_ICP_OK;
  if (const int rc = seq_corr_copy_scan(c, k, d_scan, c->stream)) return rc;
  if (const int rc = seq_corr_copy_records(c, k)) return rc;
  seq_corr_note(c, k, H, guess, ep);
  return SO_ICP_OK;
}

void seq_corr_fail(so_icp_ctx* c) {
  if (!c->seq_corr) return;
  for (so_icp_ctx::CorrLast& r : c->seq_corr->rec) r.valid = false;
}

}  // namespace soicp::host

namespace {

using KeptSets = so_icp_ctx::KeptSets;

// What differs between the batch's and the run's three C entries: their names and the words of their messages, the selection's limit, and
// what an export reports of an entry without a set
struct SelectionNames {
  const char *keep, *exports, *sums;  // the entries
  const char* sharded;                // why the switch is refused on a sharded context
  const char* noun;                   // an entry of the selection, in messages
  const char* outside;                // a selection index out of range
  const char* max_name; int max_selection;
  const char* status_room;            // what status_out must hold
  bool points_without_set;            // info[k].n_points of an entry without a set: the length of its status row (a run's frames differ in
                                      // length; a batch reports nothing of such an entry)
};
const SelectionNames kBatch = {"so_icp_keep_batch_correspondences", "so_icp_batch_correspondences", "so_icp_batch_correspondence_sums",
                               "so_icp_register_batch needs the whole map on one device (world_size == 1)", "hypothesis",
                               "a hypothesis index lies outside the last batch (0 .. n_hyp - 1)", "SO_ICP_BATCH_MAX_SELECTION", SO_ICP_BATCH_MAX_SELECTION,
                               "n_sel x the points of the batch's scan", false};
const SelectionNames kRun = {"so_icp_keep_sequence_correspondences", "so_icp_sequence_correspondences", "so_icp_sequence_correspondence_sums",
                             "a sharded context (world_size > 1) keeps its correspondences per rank", "frame",
                             "a frame index lies outside the last run (0 .. count - 1)", "SO_ICP_SEQUENCE_MAX_SELECTION", SO_ICP_SEQUENCE_MAX_SELECTION,
                             "the points of all selected frames", true};

// The exports' own buffers, one set of them per kept set: nothing here is written by another entry, and the exports write no other
// entry's buffers
struct SelectionExportState {
  DevBuf records, status;
  DevBuf tables;     // entries n_sel x CorrSelEntry | tile_first n_sel + 1
  DevBuf small;      // {ticket, -, -, -} | counts n_sel | tile sums of the cost n_tiles | look-back words n_tiles
  PinnedBuf h_tables, h_small;
  // the sums
  DevBuf sums_tables;  // poses n_sel x n_poses x 7 | histograms n_sel x 16 | entries | tile_first
  DevBuf partials, sums;
  PinnedBuf h_io;      // the tables on their way in, the sums on their way out
  ~SelectionExportState() {
    for (DevBuf* b : {&records, &status, &tables, &small, &sums_tables, &partials, &sums}) b->release();
  }
};

SelectionExportState& export_state_of(std::shared_ptr<void>& slot) {
  if (!slot) slot = std::make_shared<SelectionExportState>();
  return *static_cast<SelectionExportState*>(slot.get());
}

size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

// the set an export reads: nullptr when the switch is off or the last batch / run left none
const KeptSets* kept_set(bool keep, const std::unique_ptr<KeptSets>& K) { return (keep && K && K->valid) ? K.get() : nullptr; }

int check_selection(so_icp_ctx* c, const std::string& entry, const SelectionNames& names, const int32_t* sel, int n_sel, int n_entries) {
  if (batch_selection_first_bad(sel, n_sel, n_entries) >= 0) return fail(c, SO_ICP_E_INVALID, entry + ": " + names.outside);
  return SO_ICP_OK;
}

// The entry and tile tables of a selection at `dst` (entries, then tile_first): an entry without a set has no point and no tile.
// info (nullable): n_sel, the export's evaluation poses.  -> the tiles of the selection
uint32_t fill_tables(const KeptSets& K, const int32_t* sel, int n_sel, const so_icp_correspondence_info* info, const uint64_t* first_record,
                     const uint64_t* first_status, uint8_t* dst) {
  std::vector<uint32_t> points((size_t)n_sel), tile_first((size_t)n_sel + 1);
  for (int k = 0; k < n_sel; ++k) {
    const size_t e = (size_t)(sel ? sel[k] : k);
    const so_icp_ctx::CorrLast& L = K.rec[e];
    CorrSelEntry E{};
    E.at = K.at[e]; E.scan_at = K.scan_at[e];
    E.rec_first = first_record ? first_record[k] : 0;
    E.status_first = first_status ? first_status[k] : 0;
    E.a2 = L.a2; E.variant = L.variant;
    const double identity[7] = {0, 0, 0, 0, 0, 0, 1};
    std::memcpy(E.pose, (L.valid && info) ? info[k].pose_eval : identity, sizeof(E.pose));
    E.n = points[(size_t)k] = L.valid ? (uint32_t)K.n[e] : 0u;
    std::memcpy(dst + (size_t)k * sizeof(CorrSelEntry), &E, sizeof(E));
  }
  const uint32_t tiles = selection_tile_table(points.data(), (uint32_t)n_sel, kCorrTile, tile_first.data());
  std::memcpy(dst + (size_t)n_sel * sizeof(CorrSelEntry), tile_first.data(), tile_first.size() * 4);
  return tiles;
}

// n_largest: the points of the largest selected entry that has a set
CorrSelIn kernel_input(const KeptSets& K, const uint8_t* d_tables, int n_sel, uint32_t tiles, size_t n_largest) {
  CorrSelIn in;
  in.scan = K.scan.as<float>();
  in.corr = CorrBuffers{K.nd.as<double4>(), K.coeff.as<double>(), K.status.as<uint8_t>()};
  in.entries = reinterpret_cast<const CorrSelEntry*>(d_tables);
  in.tile_first = reinterpret_cast<const uint32_t*>(d_tables + (size_t)n_sel * sizeof(CorrSelEntry));
  in.n_sel = (uint32_t)n_sel; in.n_tiles = tiles; in.max_tiles = correspondence_workgroups((uint32_t)n_largest);
  return in;
}

int keep_selection(so_icp_ctx* c, const SelectionNames& names, int on, bool& keep, std::unique_ptr<KeptSets>& K, std::shared_ptr<void>& state) {
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, std::string(names.keep) + ": " + names.sharded);
  keep = on != 0;
  if (!keep) {  // (the set and the exports' buffers go with it)
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    K.reset(); state.reset();
  }
  return SO_ICP_OK;
}

// so_icp_batch_correspondences / so_icp_sequence_correspondences behind the NULL check of the context.  K: kept_set(); first_status:
// nullable (the batch's entry has no such output: its rows are n_sel x the batch's points)
int export_selection(so_icp_ctx* c, const SelectionNames& names, const KeptSets* K, std::shared_ptr<void>& state, const int32_t* sel, int n_sel,
                     const double* poses, so_icp_correspondence* records, size_t cap_records, uint64_t* first_record, uint8_t* status_out,
                     size_t cap_status, uint64_t* first_status, void** d_records_out, so_icp_correspondence_info* info) {
  static_assert(sizeof(so_icp_correspondence) == kCorrRecordBytes, "the kernel writes so_icp_correspondence records");
  const std::string entry = names.exports;
  if (n_sel < 0 || n_sel > names.max_selection) return fail(c, SO_ICP_E_INVALID, entry + ": n_sel must be 0 .. " + names.max_name);
  if (info) std::memset(info, 0, (size_t)n_sel * sizeof(*info));
  if (first_record) std::memset(first_record, 0, ((size_t)n_sel + 1) * sizeof(*first_record));
  if (first_status) std::memset(first_status, 0, ((size_t)n_sel + 1) * sizeof(*first_status));
  if (d_records_out) *d_records_out = nullptr;
  NEED_DEVICE(c);
  if (!K || !n_sel) return SO_ICP_OK;
  if (const int rc = check_selection(c, entry, names, sel, n_sel, K->entries())) return rc;
  const size_t S = (size_t)n_sel;
  std::vector<uint64_t> local_status;
  if (!first_status) { local_status.assign(S + 1, 0); first_status = local_status.data(); }
  const uint64_t status_bytes = sequence_status_ranges(K->n.data(), sel, n_sel, first_status);
  if (status_out && cap_status < status_bytes) {
    std::memset(first_status, 0, (S + 1) * sizeof(*first_status));
    return fail(c, SO_ICP_E_INVALID, entry + ": status_out needs cap_status >= " + names.status_room);
  }
  std::vector<so_icp_correspondence_info> local_info;
  if (!info) { local_info.assign(S, so_icp_correspondence_info{}); info = local_info.data(); }
  std::vector<uint64_t> local_first;
  if (!first_record) { local_first.assign(S + 1, 0); first_record = local_first.data(); }
  // the record ranges, from the counts the entries reported (reg_plan.h)
  std::vector<uint32_t> accepted((size_t)K->entries());
  std::vector<uint8_t> valid((size_t)K->entries());
  for (int e = 0; e < K->entries(); ++e) { accepted[(size_t)e] = K->rec[(size_t)e].n_accepted; valid[(size_t)e] = K->rec[(size_t)e].valid ? 1 : 0; }
  const uint64_t total = batch_record_ranges(accepted.data(), valid.data(), sel, n_sel, first_record);
  size_t n_largest = 0;  // points of the largest selected entry that has a set
  for (int k = 0; k < n_sel; ++k) {
    const size_t e = (size_t)(sel ? sel[k] : k);
    const so_icp_ctx::CorrLast& L = K->rec[e];
    if (L.valid || names.points_without_set) info[k].n_points = K->n[e];
    if (!L.valid) continue;
    n_largest = std::max(n_largest, K->n[e]);
    info[k].valid = 1; info[k].outer_iteration = L.outer_iteration;
    std::memcpy(info[k].pose_fit, L.pose_fit, sizeof(info[k].pose_fit));
    std::memcpy(info[k].pose_eval, poses ? poses + 7 * (size_t)k : L.pose_eval, sizeof(info[k].pose_eval));
  }
  if (!n_largest) {  // (no selected entry with a set and a point: rows of 254 for the entries without a set, nothing for the empty scans)
    if (status_out && status_bytes) std::memset(status_out, 254, (size_t)status_bytes);
    return SO_ICP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  SelectionExportState& st = export_state_of(state);
  const size_t table_bytes = S * sizeof(CorrSelEntry) + (S + 1) * 4;
  HIP_TRY(c, st.h_tables.reserve(table_bytes));
  const size_t tiles = fill_tables(*K, sel, n_sel, info, first_record, first_status, st.h_tables.p);
  const size_t counts_off = 16, cost_off = counts_off + round8(S * 4), state_off = cost_off + tiles * 8, small_bytes = state_off + tiles * 8;
  // (an entry writes at most its own points from its offset on: with room for the largest selected entry behind the last range no
  //  count, right or wrong, leaves the buffer)
  HIP_TRY(c, st.records.reserve((total + n_largest) * kCorrRecordBytes + 64));
  HIP_TRY(c, st.status.reserve((size_t)status_bytes + 64));
  HIP_TRY(c, st.tables.reserve(table_bytes));
  HIP_TRY(c, st.small.reserve(small_bytes));
  HIP_TRY(c, st.h_small.reserve(state_off));
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(st.tables.p, st.h_tables.p, table_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, small_bytes, s));
  const CorrSelIn in = kernel_input(*K, st.tables.as<uint8_t>(), n_sel, (uint32_t)tiles, n_largest);
  launch_selection_correspondences(in, st.records.as<uint8_t>(), st.status.as<uint8_t>(), reinterpret_cast<uint32_t*>(st.small.as<uint8_t>() + counts_off),
                                   reinterpret_cast<double*>(st.small.as<uint8_t>() + cost_off),
                                   reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), st.small.as<uint32_t>(), s);
  HIP_TRY(c, hipGetLastError());
  // (the copies are sized by what the entries reported; the kernel's own counts are checked against that afterwards)
  const bool want_records = records && cap_records >= total;
  if (want_records && total) HIP_TRY(c, hipMemcpyAsync(records, st.records.p, (size_t)total * kCorrRecordBytes, hipMemcpyDeviceToHost, s));
  if (status_out) HIP_TRY(c, hipMemcpyAsync(status_out, st.status.p, (size_t)status_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st.h_small.p, st.small.p, state_off, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  size_t tile0 = 0;
  for (int k = 0; k < n_sel; ++k) {
    const size_t row = (size_t)(first_status[k + 1] - first_status[k]);
    if (!info[k].valid) {  // (the kernel wrote nothing for it)
      if (status_out && row) std::memset(status_out + first_status[k], 254, row);
      continue;
    }
    const size_t nblk = correspondence_workgroups((uint32_t)row);
    uint32_t count;
    std::memcpy(&count, st.h_small.p + counts_off + (size_t)k * 4, 4);
    if ((uint64_t)count != first_record[k + 1] - first_record[k])
      return fail(c, SO_ICP_E_HIP, entry + ": the status bytes of " + names.noun + " " + std::to_string(sel ? sel[k] : k) +
                                       " hold another number of accepted points than it reported");
    double cost = 0;  // the tiles in tile order
    for (size_t b = 0; b < nblk; ++b) { double t; std::memcpy(&t, st.h_small.p + cost_off + (tile0 + b) * 8, 8); cost += t; }
    tile0 += nblk;
    info[k].n_accepted = count; info[k].cost = cost;
  }
  if (d_records_out) *d_records_out = st.records.p;
  return SO_ICP_OK;
}

// so_icp_batch_correspondence_sums / so_icp_sequence_correspondence_sums behind the NULL check of the context
int sum_selection(so_icp_ctx* c, const SelectionNames& names, const KeptSets* K, std::shared_ptr<void>& state, const int32_t* sel, int n_sel,
                  const double* poses, int n_poses, so_icp_sums* sums_out) {
  const std::string entry = names.sums;
  if (n_sel < 0 || n_sel > names.max_selection) return fail(c, SO_ICP_E_INVALID, entry + ": n_sel must be 0 .. " + names.max_name);
  if (n_poses < 1 || n_poses > SO_ICP_SUMS_MAX_POSES) return fail(c, SO_ICP_E_INVALID, entry + ": n_poses must be 1 .. SO_ICP_SUMS_MAX_POSES");
  if (!n_sel) return SO_ICP_OK;
  if (!poses || !sums_out) return fail(c, SO_ICP_E_INVALID, entry + ": poses and sums_out must not be NULL");
  const size_t S = (size_t)n_sel, P = (size_t)n_poses;
  std::memset(sums_out, 0, S * P * sizeof(so_icp_sums));
  NEED_DEVICE(c);
  if (!K) return SO_ICP_OK;
  if (const int rc = check_selection(c, entry, names, sel, n_sel, K->entries())) return rc;
  auto entry_of = [&](int k) { return (size_t)(sel ? sel[k] : k); };
  auto record_of = [&](int k) -> const so_icp_ctx::CorrLast& { return K->rec[entry_of(k)]; };
  int n_valid = 0;
  size_t n_largest = 0;  // points of the largest selected entry that has a set
  for (int k = 0; k < n_sel; ++k)
    if (record_of(k).valid) { ++n_valid; n_largest = std::max(n_largest, K->n[entry_of(k)]); }
  if (!n_valid) return SO_ICP_OK;
  if (!n_largest) {  // kept sets of no points: zero sums, their histograms
    for (int k = 0; k < n_sel; ++k) {
      if (!record_of(k).valid) continue;
      for (size_t j = 0; j < P; ++j)
        for (int w = 0; w < 16; ++w) sums_out[(size_t)k * P + j].hist[w] = (double)record_of(k).hist[w];
    }
    return SO_ICP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  SelectionExportState& st = export_state_of(state);
  const size_t off_hist = S * P * 7 * sizeof(double), off_entries = off_hist + S * 16 * sizeof(double);
  const size_t table_bytes = off_entries + S * sizeof(CorrSelEntry) + (S + 1) * 4;
  const size_t sums_bytes = S * P * sizeof(so_icp_sums);
  HIP_TRY(c, st.h_io.reserve(std::max(table_bytes, sums_bytes)));
  std::memcpy(st.h_io.p, poses, off_hist);
  for (int k = 0; k < n_sel; ++k) {
    const so_icp_ctx::CorrLast& L = record_of(k);
    double hist[16];
    for (int w = 0; w < 16; ++w) hist[w] = L.valid ? (double)L.hist[w] : 0.0;
    std::memcpy(st.h_io.p + off_hist + (size_t)k * sizeof(hist), hist, sizeof(hist));
  }
  const size_t tiles = fill_tables(*K, sel, n_sel, nullptr, nullptr, nullptr, st.h_io.p + off_entries);
  HIP_TRY(c, st.sums_tables.reserve(table_bytes));
  HIP_TRY(c, st.sums.reserve(sums_bytes));
  HIP_TRY(c, st.partials.reserve((tiles * P + 1) * kCorrSumsAcc * sizeof(double)));
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(st.sums_tables.p, st.h_io.p, table_bytes, hipMemcpyHostToDevice, s));
  const CorrSelIn in = kernel_input(*K, st.sums_tables.as<uint8_t>() + off_entries, n_sel, (uint32_t)tiles, n_largest);
  launch_selection_correspondence_sums(in, st.sums_tables.as<double>(), (uint32_t)n_poses, reinterpret_cast<const double*>(st.sums_tables.as<uint8_t>() + off_hist),
                                       st.partials.as<double>(), st.sums.as<double>(), s);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(st.h_io.p, st.sums.p, sums_bytes, hipMemcpyDeviceToHost, s));  // (behind the table's copy in the same queue)
  HIP_TRY(c, hipStreamSynchronize(s));
  std::memcpy(sums_out, st.h_io.p, sums_bytes);
  for (int k = 0; k < n_sel; ++k) {
    const so_icp_ctx::CorrLast& L = record_of(k);
    if (!L.valid) { std::memset(sums_out + (size_t)k * P, 0, P * sizeof(so_icp_sums)); continue; }
    for (size_t j = 0; j < P; ++j)
      if (sums_out[(size_t)k * P + j].count != (double)L.n_accepted)
        return fail(c, SO_ICP_E_HIP, entry + ": the status bytes of " + names.noun + " " + std::to_string(sel ? sel[k] : k) +
                                         " hold another number of accepted points than it reported");
  }
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_keep_batch_correspondences(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  return keep_selection(c, kBatch, on, c->batch_corr_keep, c->batch_corr, c->batch_corr_state);
}

int so_icp_batch_correspondences(so_icp_ctx* c, const int32_t* hyp, int n_sel, const double* poses, so_icp_correspondence* records, size_t cap_records,
                                 uint64_t* first_record, uint8_t* status_out, size_t cap_status, void** d_records_out, so_icp_correspondence_info* info) {
  if (!c) return SO_ICP_E_INVALID;
  return export_selection(c, kBatch, kept_set(c->batch_corr_keep, c->batch_corr), c->batch_corr_state, hyp, n_sel, poses, records, cap_records,
                          first_record, status_out, cap_status, nullptr, d_records_out, info);
}

int so_icp_batch_correspondence_sums(so_icp_ctx* c, const int32_t* hyp, int n_sel, const double* poses, int n_poses, so_icp_sums* sums_out) {
  if (!c) return SO_ICP_E_INVALID;
  return sum_selection(c, kBatch, kept_set(c->batch_corr_keep, c->batch_corr), c->batch_corr_state, hyp, n_sel, poses, n_poses, sums_out);
}

int so_icp_keep_sequence_correspondences(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  return keep_selection(c, kRun, on, c->seq_corr_keep, c->seq_corr, c->seq_corr_state);
}

int so_icp_sequence_correspondences(so_icp_ctx* c, const int32_t* frames, int n_sel, const double* poses, so_icp_correspondence* records,
                                    size_t cap_records, uint64_t* first_record, uint8_t* status_out, size_t cap_status, uint64_t* first_status,
                                    void** d_records_out, so_icp_correspondence_info* info) {
  if (!c) return SO_ICP_E_INVALID;
  return export_selection(c, kRun, kept_set(c->seq_corr_keep, c->seq_corr), c->seq_corr_state, frames, n_sel, poses, records, cap_records, first_record,
                          status_out, cap_status, first_status, d_records_out, info);
}

int so_icp_sequence_correspondence_sums(so_icp_ctx* c, const int32_t* frames, int n_sel, const double* poses, int n_poses, so_icp_sums* sums_out) {
  if (!c) return SO_ICP_E_INVALID;
  return sum_selection(c, kRun, kept_set(c->seq_corr_keep, c->seq_corr), c->seq_corr_state, frames, n_sel, poses, n_poses, sums_out);
}

}  // extern "C"
