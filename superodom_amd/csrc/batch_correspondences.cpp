// batch_correspondences.cpp -- so_icp_keep_batch_correspondences, so_icp_batch_correspondences and so_icp_batch_correspondence_sums: the
// correspondence sets of so_icp_register_batch's hypotheses, read where the batch left them.  While the switch is on a batch writes the
// records of all its hypotheses into arrays the context owns (batch.cpp: the groups' kernels get those arrays as arguments, a lane
// copies its context's), keeps one packed copy of the scan and one small host record per hypothesis (so_icp_ctx::BatchCorrKept).  The
// export is one launch of corr_kernels.hip's batch_correspondences_kernel for a whole selection of hypotheses, the sums two launches of
// corr_sums_kernels.hip's batch kernels -- the single exports' text, entry by entry.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "corr_kernels.h"
#include "ctx.h"

namespace soicp::host {

int batch_corr_begin(so_icp_ctx* c, const float* d_scan, size_t n, int n_hyp, uint32_t bs) {
  if (!c->batch_corr) c->batch_corr = std::make_unique<so_icp_ctx::BatchCorrKept>();
  so_icp_ctx::BatchCorrKept& K = *c->batch_corr;
  K.valid = false; K.n = n; K.n_hyp = n_hyp; K.bs = bs;
  K.rec.assign((size_t)n_hyp, so_icp_ctx::CorrLast{});
  if (!n_hyp) { K.valid = true; return SO_ICP_OK; }  // (a batch of no hypotheses: a set nothing can be selected from)
  const size_t elems = (size_t)n_hyp * bs;
  HIP_TRY(c, K.nd.reserve(elems * sizeof(double4)));
  HIP_TRY(c, K.coeff.reserve(elems * sizeof(double)));
  HIP_TRY(c, K.status.reserve(elems));
  if (n) {
    HIP_TRY(c, K.scan.reserve(n * 12 + 64));
    HIP_TRY(c, hipMemcpyAsync(K.scan.p, d_scan, n * 12, hipMemcpyDeviceToDevice, c->stream));
  }
  return SO_ICP_OK;
}

}  // namespace soicp::host

namespace {

// The exports' own buffers: nothing here is written by another entry, and the exports write no other entry's buffers
struct BatchCorrExportState {
  DevBuf records, status;
  DevBuf tables;     // poses n_sel x 7 | record offsets n_sel | hypothesis indices n_sel
  DevBuf small;      // {ticket, -, -, -} | counts n_sel | tile sums of the cost n_sel x nblk | look-back words n_sel x nblk
  PinnedBuf h_tables, h_small;
  // so_icp_batch_correspondence_sums
  DevBuf sums_tables;  // poses n_sel x n_poses x 7 | histograms n_sel x 16 | hypothesis indices n_sel
  DevBuf partials, sums;
  PinnedBuf h_io;      // the tables on their way in, the sums on their way out
  ~BatchCorrExportState() {
    for (DevBuf* b : {&records, &status, &tables, &small, &sums_tables, &partials, &sums}) b->release();
  }
};

BatchCorrExportState* batch_export_state_of(so_icp_ctx* c) {
  if (!c->batch_corr_state) c->batch_corr_state = std::make_shared<BatchCorrExportState>();
  return static_cast<BatchCorrExportState*>(c->batch_corr_state.get());
}

size_t round8(size_t b) { return (b + 7) & ~(size_t)7; }

// the set an export reads: nullptr when the switch is off or the last batch left none
const so_icp_ctx::BatchCorrKept* kept_set(const so_icp_ctx* c) {
  return (c->batch_corr_keep && c->batch_corr && c->batch_corr->valid) ? c->batch_corr.get() : nullptr;
}

int check_selection(so_icp_ctx* c, const char* entry, const int32_t* hyp, int n_sel, int n_hyp) {
  if (batch_selection_first_bad(hyp, n_sel, n_hyp) >= 0)
    return fail(c, SO_ICP_E_INVALID, std::string(entry) + ": a hypothesis index lies outside the last batch (0 .. n_hyp - 1)");
  return SO_ICP_OK;
}

}  // namespace

extern "C" {

int so_icp_keep_batch_correspondences(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size > 1)
    return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_keep_batch_correspondences: so_icp_register_batch needs the whole map on one device (world_size == 1)");
  c->batch_corr_keep = on != 0;
  if (!c->batch_corr_keep) {  // (the set and the exports' buffers go with it)
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->batch_corr.reset(); c->batch_corr_state.reset();
  }
  return SO_ICP_OK;
}

int so_icp_batch_correspondences(so_icp_ctx* c, const int32_t* hyp, int n_sel, const double* poses, so_icp_correspondence* records, size_t cap_records,
                                 uint64_t* first_record, uint8_t* status_out, size_t cap_status, void** d_records_out, so_icp_correspondence_info* info) {
  static_assert(sizeof(so_icp_correspondence) == kCorrRecordBytes, "the kernel writes so_icp_correspondence records");
  if (!c) return SO_ICP_E_INVALID;
  if (n_sel < 0 || n_sel > SO_ICP_BATCH_MAX_SELECTION) return fail(c, SO_ICP_E_INVALID, "so_icp_batch_correspondences: n_sel must be 0 .. SO_ICP_BATCH_MAX_SELECTION");
  if (info) std::memset(info, 0, (size_t)n_sel * sizeof(*info));
  if (first_record) std::memset(first_record, 0, ((size_t)n_sel + 1) * sizeof(*first_record));
  if (d_records_out) *d_records_out = nullptr;
  NEED_DEVICE(c);
  const so_icp_ctx::BatchCorrKept* K = kept_set(c);
  if (!K || !n_sel) return SO_ICP_OK;
  if (const int rc = check_selection(c, "so_icp_batch_correspondences", hyp, n_sel, K->n_hyp)) return rc;
  const size_t n = K->n;
  if (status_out && cap_status < (size_t)n_sel * n)
    return fail(c, SO_ICP_E_INVALID, "so_icp_batch_correspondences: status_out needs cap_status >= n_sel x the points of the batch's scan");
  std::vector<so_icp_correspondence_info> local_info;
  if (!info) { local_info.assign((size_t)n_sel, so_icp_correspondence_info{}); info = local_info.data(); }
  std::vector<uint64_t> local_first;
  if (!first_record) { local_first.assign((size_t)n_sel + 1, 0); first_record = local_first.data(); }
  // the record ranges, from the counts the hypotheses reported (reg_plan.h)
  std::vector<uint32_t> accepted((size_t)K->n_hyp);
  std::vector<uint8_t> valid((size_t)K->n_hyp);
  for (int h = 0; h < K->n_hyp; ++h) { accepted[(size_t)h] = K->rec[(size_t)h].n_accepted; valid[(size_t)h] = K->rec[(size_t)h].valid ? 1 : 0; }
  const uint64_t total = batch_record_ranges(accepted.data(), valid.data(), hyp, n_sel, first_record);
  int n_valid = 0;
  for (int k = 0; k < n_sel; ++k) {
    const so_icp_ctx::CorrLast& L = K->rec[(size_t)(hyp ? hyp[k] : k)];
    if (!L.valid) continue;
    ++n_valid;
    info[k].valid = 1; info[k].n_points = n; info[k].outer_iteration = L.outer_iteration;
    std::memcpy(info[k].pose_fit, L.pose_fit, sizeof(info[k].pose_fit));
    std::memcpy(info[k].pose_eval, poses ? poses + 7 * (size_t)k : L.pose_eval, sizeof(info[k].pose_eval));
  }
  if (!n || !n_valid) {  // (a batch on an empty scan: valid entries of zero counts; no valid entry: nothing was sampled)
    if (status_out && n) std::memset(status_out, 254, (size_t)n_sel * n);
    return SO_ICP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  BatchCorrExportState& st = *batch_export_state_of(c);
  const size_t nblk = correspondence_workgroups((uint32_t)n), S = (size_t)n_sel;
  const size_t off_first = S * 7 * sizeof(double), off_hyp = off_first + S * 8, table_bytes = off_hyp + S * 4;
  const size_t counts_off = 16, cost_off = counts_off + round8(S * 4), state_off = cost_off + S * nblk * 8, small_bytes = state_off + S * nblk * 8;
  // (an entry writes at most n records from its offset on: with room for n behind the last range no count, right or wrong, leaves the buffer)
  HIP_TRY(c, st.records.reserve((total + n) * kCorrRecordBytes + 64));
  HIP_TRY(c, st.status.reserve(S * n + 64));
  HIP_TRY(c, st.tables.reserve(table_bytes));
  HIP_TRY(c, st.small.reserve(small_bytes));
  HIP_TRY(c, st.h_tables.reserve(table_bytes));
  HIP_TRY(c, st.h_small.reserve(state_off));
  for (int k = 0; k < n_sel; ++k) {
    const int h = hyp ? hyp[k] : k;
    const uint32_t hw = info[k].valid ? (uint32_t)h : kCorrNoHypothesis;
    const unsigned long long at = first_record[k];
    const double identity[7] = {0, 0, 0, 0, 0, 0, 1};
    std::memcpy(st.h_tables.p + (size_t)k * 56, info[k].valid ? info[k].pose_eval : identity, 56);
    std::memcpy(st.h_tables.p + off_first + (size_t)k * 8, &at, 8);
    std::memcpy(st.h_tables.p + off_hyp + (size_t)k * 4, &hw, 4);
  }
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(st.tables.p, st.h_tables.p, table_bytes, hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(st.small.p, 0, small_bytes, s));
  CorrBatchIn in;
  in.scan = K->scan.as<float>();
  in.corr = K->slice(0);
  in.bs = K->bs; in.n = (uint32_t)n; in.n_sel = (uint32_t)n_sel;
  in.hyp = reinterpret_cast<const uint32_t*>(st.tables.as<uint8_t>() + off_hyp);
  in.a2 = K->a2; in.variant = K->variant;
  launch_batch_correspondences(in, st.tables.as<double>(), reinterpret_cast<const unsigned long long*>(st.tables.as<uint8_t>() + off_first),
                               st.records.as<uint8_t>(), st.status.as<uint8_t>(), reinterpret_cast<uint32_t*>(st.small.as<uint8_t>() + counts_off),
                               reinterpret_cast<double*>(st.small.as<uint8_t>() + cost_off),
                               reinterpret_cast<unsigned long long*>(st.small.as<uint8_t>() + state_off), st.small.as<uint32_t>(), s);
  HIP_TRY(c, hipGetLastError());
  // (the copies are sized by what the hypotheses reported; the kernel's own counts are checked against that afterwards)
  const bool want_records = records && cap_records >= total;
  if (want_records && total) HIP_TRY(c, hipMemcpyAsync(records, st.records.p, (size_t)total * kCorrRecordBytes, hipMemcpyDeviceToHost, s));
  if (status_out) HIP_TRY(c, hipMemcpyAsync(status_out, st.status.p, S * n, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(st.h_small.p, st.small.p, state_off, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (int k = 0; k < n_sel; ++k) {
    if (!info[k].valid) {  // (the kernel wrote nothing for it)
      if (status_out) std::memset(status_out + (size_t)k * n, 254, n);
      continue;
    }
    uint32_t count;
    std::memcpy(&count, st.h_small.p + counts_off + (size_t)k * 4, 4);
    if ((uint64_t)count != first_record[k + 1] - first_record[k])
      return fail(c, SO_ICP_E_HIP, "so_icp_batch_correspondences: the status bytes of hypothesis " + std::to_string(hyp ? hyp[k] : k) +
                                       " hold another number of accepted points than it reported");
    double cost = 0;  // the tiles in tile order
    for (size_t b = 0; b < nblk; ++b) { double t; std::memcpy(&t, st.h_small.p + cost_off + ((size_t)k * nblk + b) * 8, 8); cost += t; }
    info[k].n_accepted = count; info[k].cost = cost;
  }
  if (d_records_out) *d_records_out = st.records.p;
  return SO_ICP_OK;
}

int so_icp_batch_correspondence_sums(so_icp_ctx* c, const int32_t* hyp, int n_sel, const double* poses, int n_poses, so_icp_sums* sums_out) {
  if (!c) return SO_ICP_E_INVALID;
  if (n_sel < 0 || n_sel > SO_ICP_BATCH_MAX_SELECTION) return fail(c, SO_ICP_E_INVALID, "so_icp_batch_correspondence_sums: n_sel must be 0 .. SO_ICP_BATCH_MAX_SELECTION");
  if (n_poses < 1 || n_poses > SO_ICP_SUMS_MAX_POSES) return fail(c, SO_ICP_E_INVALID, "so_icp_batch_correspondence_sums: n_poses must be 1 .. SO_ICP_SUMS_MAX_POSES");
  if (!n_sel) return SO_ICP_OK;
  if (!poses || !sums_out) return fail(c, SO_ICP_E_INVALID, "so_icp_batch_correspondence_sums: poses and sums_out must not be NULL");
  const size_t S = (size_t)n_sel, P = (size_t)n_poses;
  std::memset(sums_out, 0, S * P * sizeof(so_icp_sums));
  NEED_DEVICE(c);
  const so_icp_ctx::BatchCorrKept* K = kept_set(c);
  if (!K) return SO_ICP_OK;
  if (const int rc = check_selection(c, "so_icp_batch_correspondence_sums", hyp, n_sel, K->n_hyp)) return rc;
  const size_t n = K->n;
  auto record_of = [&](int k) -> const so_icp_ctx::CorrLast& { return K->rec[(size_t)(hyp ? hyp[k] : k)]; };
  int n_valid = 0;
  for (int k = 0; k < n_sel; ++k) n_valid += record_of(k).valid ? 1 : 0;
  if (!n_valid) return SO_ICP_OK;
  if (!n) {  // kept sets of no points: zero sums, their histograms
    for (int k = 0; k < n_sel; ++k) {
      if (!record_of(k).valid) continue;
      for (size_t j = 0; j < P; ++j)
        for (int w = 0; w < 16; ++w) sums_out[(size_t)k * P + j].hist[w] = (double)record_of(k).hist[w];
    }
    return SO_ICP_OK;
  }
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  BatchCorrExportState& st = *batch_export_state_of(c);
  const size_t nblk = correspondence_workgroups((uint32_t)n);
  const size_t off_hist = S * P * 7 * sizeof(double), off_hyp = off_hist + S * 16 * sizeof(double), table_bytes = off_hyp + S * 4;
  const size_t sums_bytes = S * P * sizeof(so_icp_sums);
  HIP_TRY(c, st.h_io.reserve(std::max(table_bytes, sums_bytes)));
  HIP_TRY(c, st.sums_tables.reserve(table_bytes));
  HIP_TRY(c, st.sums.reserve(sums_bytes));
  HIP_TRY(c, st.partials.reserve(S * P * nblk * kCorrSumsAcc * sizeof(double)));
  std::memcpy(st.h_io.p, poses, off_hist);
  for (int k = 0; k < n_sel; ++k) {
    const so_icp_ctx::CorrLast& L = record_of(k);
    double hist[16];
    for (int w = 0; w < 16; ++w) hist[w] = L.valid ? (double)L.hist[w] : 0.0;
    const uint32_t hw = L.valid ? (uint32_t)(hyp ? hyp[k] : k) : kCorrNoHypothesis;
    std::memcpy(st.h_io.p + off_hist + (size_t)k * sizeof(hist), hist, sizeof(hist));
    std::memcpy(st.h_io.p + off_hyp + (size_t)k * 4, &hw, 4);
  }
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(st.sums_tables.p, st.h_io.p, table_bytes, hipMemcpyHostToDevice, s));
  CorrBatchIn in;
  in.scan = K->scan.as<float>();
  in.corr = K->slice(0);
  in.bs = K->bs; in.n = (uint32_t)n; in.n_sel = (uint32_t)n_sel;
  in.hyp = reinterpret_cast<const uint32_t*>(st.sums_tables.as<uint8_t>() + off_hyp);
  in.a2 = K->a2; in.variant = K->variant;
  launch_batch_correspondence_sums(in, st.sums_tables.as<double>(), (uint32_t)n_poses, reinterpret_cast<const double*>(st.sums_tables.as<uint8_t>() + off_hist),
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
        return fail(c, SO_ICP_E_HIP, "so_icp_batch_correspondence_sums: the status bytes of hypothesis " + std::to_string(hyp ? hyp[k] : k) +
                                         " hold another number of accepted points than it reported");
  }
  return SO_ICP_OK;
}

}  // extern "C"
