// staging.cpp -- so_icp_stage_scan: the NEXT scans on their way to HBM (and binned ahead) while the current registration runs;
// the copy thread; so_icp_host_register / _alloc.  The slots, the copy queue and the switches live in so_icp_ctx (ctx.h).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>

#include "ctx.h"

namespace soicp::host {

// Slot life: StageState (ctx.h).  Everything below runs under stage_mu: so_icp_stage_scan may come from another thread than the
// registration calls.
static bool stage_any_queued(const so_icp_ctx* c) {
  for (const so_icp_ctx::StageSlot& sl : c->stage) if (sl.state == StageState::kQueued) return true;
  return false;
}
// the copy of a direct slot has left the caller's buffer (host-side wait; a no-op in steady state: the copy was enqueued
// a registration ago)
static void stage_finish_direct(so_icp_ctx::StageSlot& sl) {
  sl.deferred = false;  // (a copy that was never enqueued reads nothing)
  if (sl.tail_stream) {  // (a copy whose event was never recorded -- the registration that enqueued it failed in between: wait for the queue)
    (void)hipStreamSynchronize(sl.tail_stream);
    sl.tail_stream = nullptr; sl.prebinned = false; sl.ev_pending = false;
  }
  if (sl.ev_pending) { (void)hipEventSynchronize(sl.ev); sl.ev_pending = false; }
}
// the slot holds an announcement of this very buffer
static bool announces(const so_icp_ctx::StageSlot& sl, const float* xyz, size_t n, size_t stride_bytes) {
  return sl.src == xyz && sl.n == n && sl.stride == stride_bytes;
}
// the slot's announcement is dropped: once the copy thread has let go of it and its copy has left the caller's buffer, it is empty
static void retire_slot(std::unique_lock<std::mutex>& lk, so_icp_ctx* c, so_icp_ctx::StageSlot& sl) {
  c->stage_cv.wait(lk, [&] { return sl.state != StageState::kQueued; });
  stage_finish_direct(sl);
  sl.src = nullptr; sl.state = StageState::kEmpty;
}
// the buffers stage_prebin needs for a scan of n points, reserved by the ANNOUNCING thread (so_icp_stage_scan, under stage_mu) next to the
// slot's scan buffer: a hipMalloc / hipFree is a device-wide synchronisation and must not sit in a registration's critical path,
// where stage_prebin runs.  A failure only means "not binned ahead".
static void stage_prebin_reserve(so_icp_ctx* c, so_icp_ctx::StageSlot& sl, size_t n) {
  if (!c->prebin || !n || n >= kMaxScanPoints) return;
  if (sl.reserve_worklist(n) != hipSuccess || c->pbin.reserve(bin_table_log2(n)) != hipSuccess) (void)hipGetLastError();
}
// Binning ahead (so_icp_ctx::prebin): scan_keys -> bin_offsets -> bin_place of a scan in HBM into the slot's pb_* buffers on queue `s`,
// under `pose` -- the work list and counters the registration of that scan starts its first k-NN sweep with (MatchParams::begin).  The
// caller has reserved the slot's buffers and made `table` clean at bin_table_log2(n) (BinHashTable::ensure).  false: a launch was
// refused (the table may have been left dirty: it is cleared before its next use).
bool bin_into_slot(so_icp_ctx* c, const float* d_scan, size_t n, const double pose[7], hipStream_t s, BinHashTable& table,
                   so_icp_ctx::StageSlot& sl) {
  const BinTable bt = table.view();
  sl.pb_chunk_cap = (uint32_t)(sl.pb_chunks.cap / 4);
  launch_scan_keys(d_scan, (uint32_t)n, c->d_state, pose, 0, 0, c->d_hist, c->view, c->cfg.max_surface_features, 0, 1,
                   sl.pb_keys.as<uint32_t>(), sl.pb_vals.as<uint32_t>(), nullptr, bt, s, false, nullptr, 0, false, 0, sl.pb_ctr.as<unsigned long long>());
  launch_bin_offsets(bt, sl.pb_chunks.as<uint32_t>(), sl.pb_chunk_cap, c->d_state, s, nullptr, 0, sl.pb_ctr.as<unsigned long long>());
  launch_bin_place(bt, d_scan, (uint32_t)n, sl.pb_keys.as<uint32_t>(), sl.pb_vals.as<uint32_t>(), sl.pb_binned.as<float4>(), s);
  if (hipGetLastError() == hipSuccess) return true;
  table.log2 = 0;
  return false;
}
// bin the slot's scan on the copy queue, behind its copy; a failure only means "not binned ahead".  Runs on the registration thread,
// inside a registration: allocates nothing -- a scan whose buffers were not reserved at its announcement is not binned ahead
static void stage_prebin(so_icp_ctx* c, so_icp_ctx::StageSlot& sl, const double* pose) {
  sl.prebinned = false;
  const size_t n = sl.n;
  if (!c->prebin || !pose || !n || n >= kMaxScanPoints) return;
  const uint32_t lg = bin_table_log2(n);
  const size_t m = n + 256;
  const bool ok = sl.pb_keys.cap >= m * 4 && sl.pb_vals.cap >= m * 4 && sl.pb_chunks.cap >= m * 4 && sl.pb_binned.cap >= m * 16 && sl.pb_ctr.cap >= 64 &&
                  c->pbin.fits(lg) && c->pbin.ensure(lg, c->copy_stream) == hipSuccess;  // (a table that fits: ensure() only clears it)
  if (!ok) { (void)hipGetLastError(); c->pbin.log2 = 0; return; }
  sl.prebinned = bin_into_slot(c, sl.dev.as<float>(), n, pose, c->copy_stream, c->pbin, sl);
}
// The DMA of a direct slot in two steps (both under stage_mu): stage_issue_copy enqueues the copy, stage_tail what follows it on the
// copy queue -- the binning ahead (only when the REGISTRATION THREAD calls it from inside a registration, with that registration's
// guess: `pose`; the copy thread and the announcing thread pass nullptr -- they must not read the context's map view) and the event the consuming
// registration waits for.  A registration in flight calls them apart (the copy right behind its first launch, the tail once its
// other launches are in the queue: the copy is the long pole -- 34 us for a 131 072-point scan -- and the binning should land in
// the shadow of the first solve, not beside the second sweep); everybody else calls stage_issue = both at once.
static hipError_t stage_issue_copy(so_icp_ctx* c, so_icp_ctx::StageSlot& sl) {
  sl.deferred = false;
  sl.prebinned = false;
  const hipError_t e = hipMemcpyAsync(sl.dev.p, sl.src, sl.n * 12, hipMemcpyHostToDevice, c->copy_stream);
  if (e == hipSuccess) { sl.tail_stream = c->copy_stream; return e; }
  sl.state = StageState::kFailed; sl.err = std::string("so_icp_stage_scan: ") + hipGetErrorString(e);
  return e;
}
static hipError_t stage_tail(so_icp_ctx* c, so_icp_ctx::StageSlot& sl, const double* pose = nullptr) {
  if (!sl.tail_stream) return hipSuccess;
  stage_prebin(c, sl, pose);
  const hipError_t e = hipEventRecord(sl.ev, c->copy_stream);
  if (e == hipSuccess) { sl.tail_stream = nullptr; sl.ev_pending = true; return e; }
  stage_finish_direct(sl);  // (waits for the copy queue instead)
  return hipSuccess;
}
static hipError_t stage_issue(so_icp_ctx* c, so_icp_ctx::StageSlot& sl) {
  const hipError_t e = stage_issue_copy(c, sl);
  return e == hipSuccess ? stage_tail(c, sl) : e;
}
// WHEN a DMA-staged scan travels.  A copy that is enqueued while the registration thread is enqueuing its launches slows
// them down: the command processor fetches every dispatch packet and its arguments from host memory over the same PCIe link
// the copy saturates with reads (measured, MI355X: registration core +10..15 us with the copy started by the announcement
// right in front of the registration call, +0 with it started here).  So an announced copy waits for the registration in
// flight to have its launches in the queue -- the host then idles for tens of microseconds, waiting for the first solve's
// report -- and is enqueued from there.  Without a registration to piggy-back on, the copy thread enqueues it after 300 us.
void stage_issue_deferred(so_icp_ctx* c, const double* prebin_pose) {
  if (!c->stage_started) return;
  std::lock_guard<std::mutex> lk(c->stage_mu);
  for (so_icp_ctx::StageSlot& sl : c->stage) {
    if (sl.state == StageState::kReady && sl.deferred) { if (stage_issue_copy(c, sl) == hipSuccess) (void)stage_tail(c, sl, prebin_pose); }
    else if (sl.state == StageState::kReady && sl.tail_stream) (void)stage_tail(c, sl, prebin_pose);
  }
}
void stage_issue_deferred_copy(so_icp_ctx* c) {  // (the registration in flight: copy now, stage_issue_deferred for the rest later)
  if (!c->stage_started) return;
  std::lock_guard<std::mutex> lk(c->stage_mu);
  for (so_icp_ctx::StageSlot& sl : c->stage) if (sl.state == StageState::kReady && sl.deferred) (void)stage_issue_copy(c, sl);
}
static bool host_range_registered(const so_icp_ctx* c, const void* p, size_t bytes) {
  const char* q = static_cast<const char*>(p);
  for (const so_icp_ctx::HostRange& r : c->host_ranges) if (q >= r.p && q + bytes <= r.p + r.bytes) return true;
  return false;
}

// Copy thread: one per context, started on first use, for sources that are NOT registered host memory.  Pack (strided input,
// e.g. 32-byte pcl::PointXYZI) into the slot's pinned buffer, hipMemcpyAsync to the slot's HBM buffer, wait, mark the slot
// ready.  A copy from pinned memory runs on an SDMA engine, whereas the runtime may serve a pageable source with a blit
// kernel that competes for compute units with the persistent solve launch of the registration in flight.
static void stage_worker(so_icp_ctx* c) {
  (void)hipSetDevice(c->cfg.device_id);
  std::unique_lock<std::mutex> lk(c->stage_mu);
  for (;;) {
    if (!(c->stage_quit || stage_any_queued(c))) {
      // DMA-staged scans waiting for a registration to enqueue them (stage_issue_deferred): after 300 us this thread does it
      {
        const auto now = std::chrono::steady_clock::now();
        bool waiting = false;
        auto deadline = now + std::chrono::hours(1);
        for (so_icp_ctx::StageSlot& q : c->stage) {
          if (!(q.state == StageState::kReady && q.deferred)) continue;
          const auto due = q.t_announced + std::chrono::microseconds(300);
          if (due <= now) (void)stage_issue(c, q); else { waiting = true; deadline = std::min(deadline, due); }
        }
        if (waiting) {
          c->stage_pending.store(0, std::memory_order_relaxed);
          c->stage_timed.store(true);
          c->stage_parked.store(true);
          c->stage_cv.wait_until(lk, deadline, [&] { return c->stage_quit || stage_any_queued(c); });
          c->stage_parked.store(false);
          c->stage_timed.store(false);
          continue;
        }
      }
      // Nothing queued.  A registration stream announces the next scan within a few hundred microseconds: spin that long
      // on the pending counter (no futex wake-up on the announcing thread's path), then park on the condition variable
      // (a 10 Hz node finds the thread parked and pays one notify per frame).
      c->stage_pending.store(0, std::memory_order_relaxed);
      lk.unlock();
      const auto t0 = std::chrono::steady_clock::now();
      bool got = false;
      while (std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(400)) {
        if (c->stage_pending.load(std::memory_order_acquire) > 0) { got = true; break; }
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        std::this_thread::yield();
#endif
      }
      lk.lock();
      if (!got) {
        auto any_deferred = [&] { for (const so_icp_ctx::StageSlot& q : c->stage) if (q.state == StageState::kReady && q.deferred) return true; return false; };
        c->stage_parked.store(true);
        c->stage_cv.wait(lk, [&] { return c->stage_quit || stage_any_queued(c) || any_deferred(); });
        c->stage_parked.store(false);
      }
      continue;
    }
    if (c->stage_quit) return;
    so_icp_ctx::StageSlot* pick = nullptr;  // oldest queued announcement first
    for (so_icp_ctx::StageSlot& q : c->stage) if (q.state == StageState::kQueued && (!pick || q.seq < pick->seq)) pick = &q;
    so_icp_ctx::StageSlot& sl = *pick;
    const float* src = sl.src; const size_t n = sl.n, stride = sl.stride; const unsigned long long seq = sl.seq;
    lk.unlock();
    std::string err;
    hipError_t e = sl.dev.reserve((n + 64) * 12);
    if (e == hipSuccess && n) {
      if (sl.pinned_cap < n * 12) {
        if (sl.pinned) (void)hipHostFree(sl.pinned);
        sl.pinned = nullptr; sl.pinned_cap = 0;
        e = hipHostMalloc(reinterpret_cast<void**>(&sl.pinned), n * 12 + 4096);
        if (e == hipSuccess) sl.pinned_cap = n * 12 + 4096;
      }
      // pack and copy in pieces of 16 384 points (192 KB): the DMA of a piece runs while the next one is being packed, so a
      // scan is in HBM after max(pack, DMA) + one piece instead of pack + DMA (it matters for the one copy nothing hides:
      // the first of a run)
      const size_t sf = stride / 4, piece = 16384;
      for (size_t i0 = 0; i0 < n && e == hipSuccess; i0 += piece) {
        const size_t m = std::min(piece, n - i0);
        float* dst = sl.pinned + 3 * i0;
        if (sf == 3) std::memcpy(dst, src + 3 * i0, m * 12);
        else for (size_t i = 0; i < m; ++i) { const float* p = src + (i0 + i) * sf; dst[3 * i] = p[0]; dst[3 * i + 1] = p[1]; dst[3 * i + 2] = p[2]; }
        e = hipMemcpyAsync(sl.dev.as<float>() + 3 * i0, dst, m * 12, hipMemcpyHostToDevice, c->copy_stream);
      }
      if (e == hipSuccess) e = hipStreamSynchronize(c->copy_stream);
    }
    if (e != hipSuccess) err = std::string("so_icp_stage_scan: ") + hipGetErrorString(e);
    lk.lock();
    if (sl.seq == seq && sl.state == StageState::kQueued) { sl.state = err.empty() ? StageState::kReady : StageState::kFailed; sl.err = err; }
    c->stage_cv.notify_all();
  }
}

// The staged copy of (xyz, n, stride) -- the NEWEST announcement of that buffer --, waiting for the copy thread if it is still
// on its way; nullptr = not staged.  A staged copy is consumed by the call that takes it: the caller may refill the same host
// buffer for a later frame, and a later call without a new so_icp_stage_scan must not see the old contents.  (The HBM buffer
// itself stays valid until the slot is staged again, i.e. for the whole call that took it.)  A copy that the announcing
// thread enqueued itself (registered host memory) is awaited by the registration's stream, not by the host.
static const float* take_staged(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, int* rc) {
  *rc = SO_ICP_OK;
  std::unique_lock<std::mutex> lk(c->stage_mu);
  if (!c->stage_started) return nullptr;
  so_icp_ctx::StageSlot* best = nullptr;
  for (so_icp_ctx::StageSlot& sl : c->stage) {
    if (sl.state == StageState::kEmpty || sl.state == StageState::kInUse || !announces(sl, xyz, n, stride_bytes)) continue;
    if (sl.seq < c->stage_consumed_seq) {
      // announced before a scan that has been consumed since: its frame was skipped, and the caller may have refilled the
      // buffer meanwhile (allowed once a later so_icp_stage_scan has returned) -- never served
      retire_slot(lk, c, sl);
      continue;
    }
    if (!best || sl.seq > best->seq) best = &sl;
  }
  if (!best) return nullptr;
  for (so_icp_ctx::StageSlot& sl : c->stage) {  // older announcements of the same buffer: superseded
    if (&sl == best || sl.state == StageState::kEmpty || sl.state == StageState::kInUse || !announces(sl, xyz, n, stride_bytes)) continue;
    retire_slot(lk, c, sl);
  }
  so_icp_ctx::StageSlot& sl = *best;
  if (sl.state == StageState::kQueued) {
    const auto t0 = std::chrono::steady_clock::now();
    c->stage_cv.wait(lk, [&] { return sl.state != StageState::kQueued; });
    c->timing.stage_wait_ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  const StageState state = sl.state;
  sl.src = nullptr;
  if (state == StageState::kReady) {
    if (sl.deferred) {  // (no registration came by to enqueue it: the first scan of a run)
      sl.src = xyz;
      if (stage_issue(c, sl) != hipSuccess) { c->err = sl.err; *rc = SO_ICP_E_HIP; sl.src = nullptr; sl.state = StageState::kEmpty; return nullptr; }
      sl.src = nullptr;
    }
    if (sl.tail_stream) (void)stage_tail(c, sl);  // (no registration finished what it had begun: not binned ahead)
    // (in a stream of registrations the copy ended long ago -- it was enqueued a registration earlier: then no barrier packet
    //  in front of this registration's first kernel either)
    if (sl.ev_pending && hipEventQuery(sl.ev) == hipSuccess) sl.ev_pending = false;
    else (void)hipGetLastError();
    if (sl.ev_pending && hipStreamWaitEvent(c->stream, sl.ev, 0) != hipSuccess) {
      (void)hipGetLastError();
      stage_finish_direct(sl);  // (cannot order the streams on the device: wait here)
    }
    sl.state = StageState::kInUse; c->stage_in_use = &sl; c->stage_consumed_seq = sl.seq;
    return sl.dev.as<float>();  // (so_icp_stage_scan -- possibly on another thread -- leaves a slot in use alone)
  }
  sl.state = StageState::kEmpty;
  if (state == StageState::kFailed) { c->err = sl.err; *rc = SO_ICP_E_HIP; }
  return nullptr;
}
// A call that reads (xyz, n, stride) itself -- map seeding -- without consuming a staged copy of it: the copy is dropped, so that
// a later frame whose buffer happens to have the same address and size is never served the old contents.
void drop_staged(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
  std::unique_lock<std::mutex> lk(c->stage_mu);
  if (!c->stage_started) return;
  for (so_icp_ctx::StageSlot& sl : c->stage) {
    if (sl.state == StageState::kEmpty || sl.state == StageState::kInUse || !announces(sl, xyz, n, stride_bytes)) continue;
    retire_slot(lk, c, sl);
  }
}
void release_staged(so_icp_ctx* c) {
  if (!c->stage_in_use) return;
  std::lock_guard<std::mutex> lk(c->stage_mu);
  c->stage_in_use->ev_pending = false;  // (the registration that read the slot has completed, and the copy before it)
  c->stage_in_use->state = StageState::kEmpty;
  c->stage_in_use = nullptr;
}

// the scan of this call in HBM: the staged copy when the caller announced it, else a plain upload into d_scan_own
// (enqueued on the registration's own stream in front of its kernels: no host-side wait)
int resolve_scan(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, const float** d_scan) {
  int rc = SO_ICP_OK;
  c->scan_staged = false;
  if (const float* staged = take_staged(c, xyz, n, stride_bytes ? stride_bytes : 12, &rc)) { c->scan_staged = true; *d_scan = staged; return SO_ICP_OK; }
  if (rc) return rc;
  rc = upload_scan_impl(c, xyz, n, stride_bytes, c->d_scan_own, /*wait=*/false);
  *d_scan = c->d_scan_own.as<float>();
  return rc;
}

}  // namespace soicp::host

extern "C" {

int so_icp_stage_scan(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
  if (!c || (!xyz && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4 && stride_bytes != SIZE_MAX) return fail(c, SO_ICP_E_INVALID, "stride_bytes must be a multiple of 4");
  bool queued = false, dma_only = false;
  {
    // (this entry point may be called from ANOTHER thread than the registration calls -- the node's feature callback --,
    //  so everything it touches lives under stage_mu)
    std::unique_lock<std::mutex> lk(c->stage_mu);
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    if (!c->stage_started) {
      HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
      c->stage_thread = std::thread(stage_worker, c);
      c->stage_started = true;
    }
    // The same buffer announced again supersedes its older copy (so_icp.h: this is also how a caller takes a staged buffer
    // back -- so_icp_stage_cancel); failed slots are recycled.
    for (so_icp_ctx::StageSlot& sl : c->stage) {
      if (sl.state == StageState::kQueued && sl.src == xyz) c->stage_cv.wait(lk, [&] { return sl.state != StageState::kQueued; });
      if ((sl.state == StageState::kReady && sl.src == xyz) || sl.state == StageState::kFailed) retire_slot(lk, c, sl);
    }
    if (n == 0 && stride_bytes == SIZE_MAX) return SO_ICP_OK;  // (so_icp_stage_cancel: withdraw only)
    // Slot: an empty one; else a ready copy that was announced BEFORE the scan consumed last (its frame was skipped: it would
    // never be asked for again), oldest first; else, with no registration in flight, the oldest ready copy gives way (a caller
    // that announces scans it never registers cannot block the slots).  Otherwise every slot holds a scan that is still
    // needed -- one being registered, two announced ahead of it: SO_ICP_STAGE_DECLINED (soft: that scan is uploaded by its
    // own registration call).
    so_icp_ctx::StageSlot* pick = nullptr;
    bool in_flight = false;
    for (so_icp_ctx::StageSlot& sl : c->stage) { if (sl.state == StageState::kEmpty && !pick) pick = &sl; in_flight = in_flight || sl.state == StageState::kInUse; }
    if (!pick)
      for (so_icp_ctx::StageSlot& sl : c->stage)
        if (sl.state == StageState::kReady && (sl.seq < c->stage_consumed_seq || !in_flight) && (!pick || sl.seq < pick->seq)) pick = &sl;
    if (!pick) { c->timing.stage_declined++; return SO_ICP_STAGE_DECLINED; }
    so_icp_ctx::StageSlot& sl = *pick;
    stage_finish_direct(sl);  // (an evicted copy must have left its caller's buffer)
    sl.src = xyz; sl.n = n; sl.stride = stride_bytes; sl.err.clear(); sl.seq = ++c->stage_seq; sl.ev_pending = false;
    sl.prebinned = false;  // (the slot's work list belongs to the scan it held before)
    if (stride_bytes == 12 && n && host_range_registered(c, xyz, n * 12)) {
      // registered (pinned) host memory, packed xyz: no pack, no copy thread -- the DMA reads the caller's buffer itself
      sl.state = StageState::kEmpty;  // (until the copy is enqueued: an error below leaves the slot empty)
      HIP_TRY(c, sl.dev.reserve((n + 64) * 12));
      stage_prebin_reserve(c, sl, n);  // (what the binning ahead of this scan will need: allocated here, off the registration's path)
      if (!sl.ev) HIP_TRY(c, hipEventCreateWithFlags(&sl.ev, hipEventDisableTiming));
      sl.state = StageState::kReady;
      sl.deferred = true; sl.t_announced = std::chrono::steady_clock::now(); queued = true; dma_only = true;  // (the copy thread is the time-out)
      c->timing.staged_direct++;
    } else {
      sl.state = StageState::kQueued; queued = true;
      c->timing.staged_copied++;
    }
  }
  if (queued) {
    c->stage_pending.fetch_add(1, std::memory_order_release);
    // (a copy thread in its timed wait re-reads the slots when the time is up -- at most 300 us from now, the patience a DMA
    //  announcement is entitled to anyway: no wake-up for it; a scan for the copy thread itself, or a thread parked for good, is woken)
    if (c->stage_parked.load() && !(dma_only && c->stage_timed.load())) c->stage_cv.notify_all();
  }
  return SO_ICP_OK;
}

// Pin a host buffer of the caller (hipHostRegister): scans announced from inside it with stride 12 go to HBM by DMA straight
// from the buffer.  The node side keeps its feature clouds in a few such buffers.
int so_icp_stage_cancel(so_icp_ctx* c, const float* xyz) {
  if (!c || !xyz) return SO_ICP_E_INVALID;
  if (c->host_only || !c->stage_started) return SO_ICP_OK;
  return so_icp_stage_scan(c, xyz, 0, SIZE_MAX);
}

int so_icp_host_register(so_icp_ctx* c, const void* ptr, size_t bytes) {
  if (!c || !ptr || !bytes) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  std::lock_guard<std::mutex> lk(c->stage_mu);
  if (host_range_registered(c, ptr, bytes)) return SO_ICP_OK;
  HIP_TRY(c, hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault));
  c->host_ranges.push_back(so_icp_ctx::HostRange{static_cast<const char*>(ptr), bytes, false});
  return SO_ICP_OK;
}
// Pinned host memory from the runtime's own allocator (hipHostMalloc) for the caller's clouds: the fastest DMA source.
int so_icp_host_alloc(so_icp_ctx* c, size_t bytes, void** out) {
  if (!c || !out || !bytes) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  void* p = nullptr;
  HIP_TRY(c, hipHostMalloc(&p, bytes));
  std::lock_guard<std::mutex> lk(c->stage_mu);
  c->host_ranges.push_back(so_icp_ctx::HostRange{static_cast<const char*>(p), bytes, true});
  *out = p;
  return SO_ICP_OK;
}
int so_icp_host_free(so_icp_ctx* c, void* ptr) { return so_icp_host_unregister(c, ptr); }
int so_icp_host_unregister(so_icp_ctx* c, const void* ptr) {
  if (!c || !ptr) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  std::unique_lock<std::mutex> lk(c->stage_mu);
  for (size_t i = 0; i < c->host_ranges.size(); ++i) {
    if (c->host_ranges[i].p != static_cast<const char*>(ptr)) continue;
    for (so_icp_ctx::StageSlot& sl : c->stage) stage_finish_direct(sl);  // no copy may still be reading the buffer
    if (c->copy_stream) HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    if (c->host_ranges[i].owned) HIP_TRY(c, hipHostFree(const_cast<void*>(ptr))); else HIP_TRY(c, hipHostUnregister(const_cast<void*>(ptr)));
    c->host_ranges.erase(c->host_ranges.begin() + (long)i);
    return SO_ICP_OK;
  }
  return fail(c, SO_ICP_E_INVALID, "so_icp_host_unregister / so_icp_host_free: this pointer did not come from so_icp_host_register / so_icp_host_alloc");
}

}  // extern "C"
