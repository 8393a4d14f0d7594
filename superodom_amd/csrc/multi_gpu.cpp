// multi_gpu.cpp -- several ranks: RCCL (loaded on first use), in-process shard groups, the map-count and shard exchanges of a sharded
// device map, the peer exchange between the ranks' persistent solve launches, and the shard helpers of the C ABI.
#include <dlfcn.h>
#include <unistd.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ctx.h"

namespace soicp::host {

// In-process shard group (so_icp_comm_init_inprocess): the contexts of ONE process that share a key -- one thread and one
// context per GPU, or several shard contexts on one GPU in a test -- sum their 45-double records through host memory.
// Fixed order (rank 0, 1, ...): every member receives bit-identical sums and takes identical controller decisions.
struct InprocGroup {
  std::mutex mu; std::condition_variable cv;
  int world = 0, arrived = 0, members = 0; unsigned long long generation = 0;
  // A round is identified by (kind, size): members that disagree about what is being summed -- one in the LmSums reduce, another
  // in the per-cube counts after a failed insert -- must not be paired silently; a member that returns early (a failed HIP call
  // before the exchange) or never arrives (wait_seconds) makes the round fail on every member instead of blocking the others for ever.
  int round_kind = -1; size_t round_size = 0; bool aborted = false;
  int wait_seconds = 60;  // patience with a member that has not arrived (first-call code-object load, a debugger): SOICP_GROUP_TIMEOUT_S
  std::vector<LmSums> slot; LmSums total{};
  std::vector<std::vector<int32_t>> islot; std::vector<int32_t> itotal;
  void abort_all() { std::lock_guard<std::mutex> lk(mu); aborted = true; cv.notify_all(); }
  // returns false when the round failed (mismatch, abort, or a member missing for wait_seconds): the group is unusable afterwards
  template <class Publish, class Combine>
  bool round(int kind, size_t size, Publish&& publish, Combine&& combine) {
    std::unique_lock<std::mutex> lk(mu);
    if (aborted) return false;
    if (arrived == 0) { round_kind = kind; round_size = size; }
    else if (round_kind != kind || round_size != size) { aborted = true; cv.notify_all(); return false; }
    publish();
    if (++arrived == world) {
      combine();
      arrived = 0; ++generation;
      cv.notify_all();
      return true;
    }
    const unsigned long long g = generation;
    const bool done = cv.wait_for(lk, std::chrono::seconds(wait_seconds), [&] { return generation != g || aborted; });
    if (!done || aborted) { aborted = true; cv.notify_all(); return false; }
    return true;
  }
  bool allreduce(int rank, LmSums* io) {
    const bool ok = round(0, sizeof(LmSums), [&] { slot[(size_t)rank] = *io; }, [&] {
      double* t = reinterpret_cast<double*>(&total);
      for (size_t k = 0; k < sizeof(LmSums) / sizeof(double); ++k) {
        double acc = 0;
        for (int r = 0; r < world; ++r) acc += reinterpret_cast<const double*>(&slot[(size_t)r])[k];  // fixed order: rank 0, 1, ...
        t[k] = acc;
      }
    });
    if (ok) { std::lock_guard<std::mutex> lk(mu); *io = total; }
    return ok;
  }
  // same for a vector of counters (per-cube point counts after a map insert)
  bool allreduce_i32(int rank, std::vector<int32_t>& io) {
    const bool ok = round(1, io.size(), [&] {
      if (islot.size() != (size_t)world) islot.resize((size_t)world);
      islot[(size_t)rank] = io;
    }, [&] {
      itotal.assign(io.size(), 0);
      for (int r = 0; r < world; ++r)
        for (size_t k = 0; k < io.size() && k < islot[(size_t)r].size(); ++k) itotal[k] += islot[(size_t)r][k];
    });
    if (ok) { std::lock_guard<std::mutex> lk(mu); io = itotal; }
    return ok;
  }
  // all-gather of byte strings of any length (the shards' points at a planeRes change); same discipline as above: the last
  // member to arrive assembles the result, nobody's slot is read after the round
  std::vector<std::vector<uint8_t>> bslot, ball;
  bool allgather_bytes(int rank, const std::vector<uint8_t>& mine, std::vector<std::vector<uint8_t>>& all) {
    const bool ok = round(2, 0, [&] {
      if (bslot.size() != (size_t)world) bslot.resize((size_t)world);
      bslot[(size_t)rank] = mine;
    }, [&] { ball = bslot; });
    if (ok) { std::lock_guard<std::mutex> lk(mu); all = ball; }
    return ok;
  }
};
}  // namespace soicp::host

namespace {

bool rccl_load(Rccl& r, std::string& err) {
  if (r.lib) return true;
  const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
  for (const char* n : names) { r.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL); if (r.lib) break; }
  if (!r.lib) { err = std::string("dlopen(librccl) failed: ") + dlerror(); return false; }
  r.GetUniqueId = reinterpret_cast<decltype(r.GetUniqueId)>(dlsym(r.lib, "ncclGetUniqueId"));
  r.CommInitRank = reinterpret_cast<decltype(r.CommInitRank)>(dlsym(r.lib, "ncclCommInitRank"));
  r.AllReduce = reinterpret_cast<decltype(r.AllReduce)>(dlsym(r.lib, "ncclAllReduce"));
  r.AllGather = reinterpret_cast<decltype(r.AllGather)>(dlsym(r.lib, "ncclAllGather"));
  r.CommDestroy = reinterpret_cast<decltype(r.CommDestroy)>(dlsym(r.lib, "ncclCommDestroy"));
  r.GetErrorString = reinterpret_cast<decltype(r.GetErrorString)>(dlsym(r.lib, "ncclGetErrorString"));
  if (!r.GetUniqueId || !r.CommInitRank || !r.AllReduce || !r.AllGather || !r.CommDestroy) { err = "librccl lacks a required symbol"; return false; }
  return true;
}

std::mutex g_groups_mu;
std::vector<std::pair<uint64_t, std::shared_ptr<InprocGroup>>> g_groups;

}  // namespace

namespace soicp::host {

bool group_allreduce(so_icp_ctx* c, LmSums* io) { return c->group->allreduce(c->cfg.rank, io); }
// the other members must not wait for this one's next exchange
void group_abort(so_icp_ctx* c) { if (c->group) c->group->abort_all(); }
// (so_icp_ctx::~so_icp_ctx) the registry forgets a group when its last member goes
void group_leave(so_icp_ctx* c) {
  std::lock_guard<std::mutex> lk(g_groups_mu);
  if (--c->group->members <= 0)
    for (size_t i = 0; i < g_groups.size(); ++i)
      if (g_groups[i].second == c->group) { g_groups.erase(g_groups.begin() + (long)i); break; }
}

// Sharded device map: every rank has inserted the same cloud into its shard; the per-cube point counts of the FULL map
// (get5x5LocalMapFeatureSize, LocalMap.h:292-318, and the <= 50 check of LidarSlam.cpp:113-116 read them) are the sums of
// the ranks' owned counts -- one small collective per insert (per scan), never per registration.
int exchange_map_counts(so_icp_ctx* c) {
  if (!c->dmap || !c->dmap->sharded()) return SO_ICP_OK;
  std::vector<int32_t> v;
  c->dmap->owned_counts(v);
  if (c->group) {
    if (!c->group->allreduce_i32(c->cfg.rank, v))
      return fail(c, SO_ICP_E_RCCL, "in-process group: the map-count exchange failed (a member returned early, is in another exchange, or did not arrive)");
  } else if (c->comm) {
    HIP_TRY(c, c->d_counts.reserve(v.size() * sizeof(int32_t)));
    HIP_TRY(c, hipMemcpyAsync(c->d_counts.p, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    const ncclResult_t nrc = c->rccl.AllReduce(c->d_counts.p, c->d_counts.p, v.size(), ncclInt32, ncclSum, c->comm, c->stream);
    if (nrc != ncclSuccess) return fail(c, SO_ICP_E_RCCL, std::string("ncclAllReduce(map counts): ") + (c->rccl.GetErrorString ? c->rccl.GetErrorString(nrc) : "?"));
    HIP_TRY(c, hipMemcpyAsync(v.data(), c->d_counts.p, v.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }  // (a shard context without a communicator -- tests that drive the ranks one by one -- reports its own owned counts)
  c->dmap->set_full_counts(v);
  return SO_ICP_OK;
}

// Sharded device map, planeRes change: the shards are cut along the cell grid, which follows planeRes.  Every rank hands out
// the points it owns, all ranks gather all of them (in-process group, or RCCL all-gather of the padded byte strings), and each
// re-cuts its shard on the new grid (DeviceMap::reshard).  Collective: every rank must make the same so_icp_set_resolution call.
int reshard_for_resolution(so_icp_ctx* c, float line_res, float plane_res) {
  std::vector<uint8_t> mine;
  if (c->dmap->export_owned(mine, c->err) < 0) return SO_ICP_E_HIP;
  std::vector<std::vector<uint8_t>> all;
  if (c->group) {
    if (!c->group->allgather_bytes(c->cfg.rank, mine, all))
      return fail(c, SO_ICP_E_RCCL, "in-process group: the exchange of the shards' points failed (a member returned early, is in another exchange, or did not arrive)");
  } else {
    const int W = c->cfg.world_size;
    auto nccl_fail = [&](const char* what, ncclResult_t r) { return fail(c, SO_ICP_E_RCCL, std::string(what) + ": " + (c->rccl.GetErrorString ? c->rccl.GetErrorString(r) : "?")); };
    // lengths first, then the strings padded to the longest
    std::vector<unsigned long long> len((size_t)W, 0ull);
    len[(size_t)c->cfg.rank] = mine.size();
    HIP_TRY(c, c->d_counts.reserve((size_t)W * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemcpyAsync(c->d_counts.p, len.data(), (size_t)W * sizeof(unsigned long long), hipMemcpyHostToDevice, c->stream));
    ncclResult_t r = c->rccl.AllGather(c->d_counts.as<unsigned long long>() + c->cfg.rank, c->d_counts.p, 1, ncclUint64, c->comm, c->stream);
    if (r != ncclSuccess) return nccl_fail("ncclAllGather(shard sizes)", r);
    HIP_TRY(c, hipMemcpyAsync(len.data(), c->d_counts.p, (size_t)W * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    size_t longest = 16;
    for (unsigned long long v : len) longest = std::max(longest, (size_t)v);
    longest = (longest + 15) & ~(size_t)15;
    DevBuf send, recv;
    std::vector<uint8_t> host(longest * (size_t)W);
    hipError_t e = send.reserve(longest);
    if (e == hipSuccess) e = recv.reserve(longest * (size_t)W);
    if (e == hipSuccess && !mine.empty()) e = hipMemcpyAsync(send.p, mine.data(), mine.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
      r = c->rccl.AllGather(send.p, recv.p, longest, ncclUint8, c->comm, c->stream);
      if (r != ncclSuccess) { send.release(); recv.release(); return nccl_fail("ncclAllGather(shard points)", r); }
      e = hipMemcpyAsync(host.data(), recv.p, host.size(), hipMemcpyDeviceToHost, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    send.release(); recv.release();
    HIP_TRY(c, e);
    all.resize((size_t)W);
    for (int k = 0; k < W; ++k) all[(size_t)k].assign(host.begin() + (long)(longest * (size_t)k), host.begin() + (long)(longest * (size_t)k + (size_t)len[(size_t)k]));
  }
  const int rc = c->dmap->reshard(all, line_res, plane_res, c->err);
  if (rc < 0) return map_status(rc);
  c->uploaded_version = 0;
  return SO_ICP_OK;
}

}  // namespace soicp::host

extern "C" {

int so_icp_comm_unique_id(uint8_t id[SO_ICP_UNIQUE_ID_BYTES]) {
  if (!id) return SO_ICP_E_INVALID;
  Rccl r;
  std::string err;
  if (!rccl_load(r, err)) { g_create_error = err; return SO_ICP_E_RCCL; }
  ncclUniqueId u;
  std::memset(&u, 0, sizeof(u));
  const ncclResult_t rc = r.GetUniqueId(&u);
  if (rc != ncclSuccess) { g_create_error = "ncclGetUniqueId failed"; return SO_ICP_E_RCCL; }
  std::memcpy(id, &u, SO_ICP_UNIQUE_ID_BYTES);
  return SO_ICP_OK;
}

int so_icp_comm_init(so_icp_ctx* c, const uint8_t id[SO_ICP_UNIQUE_ID_BYTES]) {
  if (!c || !id) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (!rccl_load(c->rccl, c->err)) return SO_ICP_E_RCCL;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  ncclUniqueId u;
  std::memcpy(&u, id, SO_ICP_UNIQUE_ID_BYTES);
  const ncclResult_t rc = c->rccl.CommInitRank(&c->comm, c->cfg.world_size, u, c->cfg.rank);
  if (rc != ncclSuccess) { c->comm = nullptr; return fail(c, SO_ICP_E_RCCL, std::string("ncclCommInitRank: ") + (c->rccl.GetErrorString ? c->rccl.GetErrorString(rc) : "?")); }
  return SO_ICP_OK;
}

int so_icp_comm_init_inprocess(so_icp_ctx* c, uint64_t group_key) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->comm) return fail(c, SO_ICP_E_INVALID, "so_icp_comm_init_inprocess: the context already has an RCCL communicator");
  std::lock_guard<std::mutex> lk(g_groups_mu);
  std::shared_ptr<InprocGroup> g;
  for (auto& kv : g_groups) if (kv.first == group_key) g = kv.second;
  if (!g) {
    g = std::make_shared<InprocGroup>();
    if (const char* ev = std::getenv("SOICP_GROUP_TIMEOUT_S")) { const int t = std::atoi(ev); if (t >= 1) g->wait_seconds = t; }
    g->world = c->cfg.world_size; g->slot.resize((size_t)g->world);
    g_groups.emplace_back(group_key, g);
  }
  if (g->world != c->cfg.world_size) return fail(c, SO_ICP_E_INVALID, "so_icp_comm_init_inprocess: world_size differs from the group's");
  if (g->members >= g->world) return fail(c, SO_ICP_E_INVALID, "so_icp_comm_init_inprocess: the group is complete already (use a new key)");
  g->members++;
  c->group = g;
  return SO_ICP_OK;
}

// ---- peer exchange -------------------------------------------------------------------------------------------------
namespace {
struct PeerHandle { hipIpcMemHandle_t ipc; uint64_t pid; uint64_t ptr; };
static_assert(sizeof(PeerHandle) == SO_ICP_PEER_HANDLE_BYTES, "SO_ICP_PEER_HANDLE_BYTES");
}  // namespace

int so_icp_peer_export(so_icp_ctx* c, uint8_t handle[SO_ICP_PEER_HANDLE_BYTES]) {
  if (!c || !handle) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (c->cfg.world_size < 2 || c->cfg.world_size > kPeerMaxWorld) return fail(c, SO_ICP_E_UNSUPPORTED, "peer exchange: world_size must be 2..8");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  PeerHandle h;
  std::memset(&h, 0, sizeof(h));
  if (!c->peer_own) {
    // memory another device writes while a kernel of this one polls it: uncached (else fine-grained) device memory
    hipError_t e = hipExtMallocWithFlags(&c->peer_own, kPeerInboxBytes, hipDeviceMallocUncached);
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipExtMallocWithFlags(&c->peer_own, kPeerInboxBytes, hipDeviceMallocFinegrained); }
    if (e != hipSuccess) { (void)hipGetLastError(); e = hipMalloc(&c->peer_own, kPeerInboxBytes); }
    if (e != hipSuccess) { c->peer_own = nullptr; return fail(c, SO_ICP_E_HIP, std::string("peer exchange: inbox allocation: ") + hipGetErrorString(e)); }
  }
  // A (new) handshake starts from an empty inbox -- stale pass records and self-test chunks of an earlier connection must not
  // satisfy the polls of this one -- and from pass number zero on every rank.  The exchange of the handles that follows
  // is the barrier between these clears and the first remote store.
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemset(c->peer_own, 0, kPeerInboxBytes));
  HIP_TRY(c, hipMemset(&c->d_state->peer_seq, 0, sizeof(unsigned long long)));
  c->peer_on = false; c->peer_connected = false;
  if (hipIpcGetMemHandle(&h.ipc, c->peer_own) != hipSuccess) {
    (void)hipGetLastError();  // contexts of ONE process need no IPC handle (pid + pointer below); across processes connect() will refuse
    std::memset(&h.ipc, 0, sizeof(h.ipc));
  }
  h.pid = (uint64_t)getpid(); h.ptr = (uint64_t)(uintptr_t)c->peer_own;
  std::memcpy(handle, &h, sizeof(h));
  return SO_ICP_OK;
}

int so_icp_peer_connect(so_icp_ctx* c, const uint8_t* handles, int* self_test_ok) {
  if (!c || !handles || !self_test_ok) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  *self_test_ok = 0;
  if (!c->peer_own) return fail(c, SO_ICP_E_INVALID, "so_icp_peer_connect: call so_icp_peer_export first");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  const int world = c->cfg.world_size;
  for (int r = 0; r < world; ++r) {
    PeerHandle h;
    std::memcpy(&h, handles + (size_t)r * SO_ICP_PEER_HANDLE_BYTES, sizeof(h));
    if (r == c->cfg.rank) { c->peer_inbox[r] = c->peer_own; continue; }
    if (h.pid == (uint64_t)getpid()) { c->peer_inbox[r] = (void*)(uintptr_t)h.ptr; continue; }  // same address space
    void* p = nullptr;
    const hipError_t e = hipIpcOpenMemHandle(&p, h.ipc, hipIpcMemLazyEnablePeerAccess);
    if (e != hipSuccess) { (void)hipGetLastError(); c->err = std::string("peer exchange: hipIpcOpenMemHandle(rank ") + std::to_string(r) + "): " + hipGetErrorString(e); return SO_ICP_OK; }  // self_test_ok stays 0
    c->peer_inbox[r] = p; c->peer_opened[r] = true;
  }
  c->peer_connected = true;
  // self-test with the very stores / loads of the solve's exchange (every rank runs it; waits up to 2 s for the others)
  int32_t* d_ok = reinterpret_cast<int32_t*>(c->d_fbcount);
  HIP_TRY(c, hipMemsetAsync(d_ok, 0, 4, c->stream));
  launch_peer_selftest(c->peer_inbox, c->cfg.rank, world, 0x7E570000u + (++c->peer_connects & 0xFFFFu), d_ok, c->stream);  // (every rank connects equally often)
  HIP_TRY(c, hipMemcpyAsync(c->h_u32, d_ok, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *self_test_ok = c->h_u32[0] == 1 ? 1 : 0;
  if (!*self_test_ok) c->err = "peer exchange: self-test chunks did not arrive from every rank";
  return SO_ICP_OK;
}

int so_icp_peer_enable(so_icp_ctx* c, int on) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (on && !c->peer_connected) return fail(c, SO_ICP_E_INVALID, "so_icp_peer_enable: not connected");
  c->peer_on = on != 0;
  return SO_ICP_OK;
}

int so_icp_cells_per_cube(float plane_res, double* cell_size) { return cells_per_cube(plane_res, cell_size); }

int so_icp_shard_owner_of_point(const float p[3], const int origin[3], float plane_res, int world_size) {
  if (!p || !origin) return SO_ICP_E_INVALID;
  const int ci = cube_coord((double)p[0], origin[0]), cj = cube_coord((double)p[1], origin[1]), ck = cube_coord((double)p[2], origin[2]);
  if (!(ci >= 0 && ci < kMapW && cj >= 0 && cj < kMapH && ck >= 0 && ck < kMapD)) return 0;  // counted by rank 0
  double cell;
  const int nc = cells_per_cube(plane_res, &cell);
  const int w[3] = {ci - origin[0], cj - origin[1], ck - origin[2]};
  int g[3];
  for (int a = 0; a < 3; ++a) {
    const int v = (int)std::floor(((double)p[a] - (w[a] * kCube - kHalfCube)) * (1.0 / cell));
    g[a] = v < 0 ? 0 : (v >= nc ? nc - 1 : v);
  }
  return shard_owner_of_cell(w[0], w[1], w[2], g[0], g[1], g[2], world_size);
}

int so_icp_shard_histogram(const float* scan_xyz, size_t n, size_t stride_bytes, const double pose[7], const int origin[3], float plane_res,
                           int world_size, int64_t* counts) {
  if ((!scan_xyz && n) || !pose || !origin || !counts || world_size < 1) return SO_ICP_E_INVALID;
  if (stride_bytes == 0) stride_bytes = 12;
  if (stride_bytes % 4) return SO_ICP_E_INVALID;
  const size_t sf = stride_bytes / 4;
  for (int r = 0; r < world_size; ++r) counts[r] = 0;
  for (size_t i = 0; i < n; ++i) {  // the queries' world positions exactly as scan_keys_kernel forms them (LidarSlam.cpp:397-398, 728-731)
    double wx, wy, wz;
    quat_rotate<double>(pose + 3, (double)scan_xyz[i * sf], (double)scan_xyz[i * sf + 1], (double)scan_xyz[i * sf + 2], wx, wy, wz);
    const float q[3] = {(float)(wx + pose[0]), (float)(wy + pose[1]), (float)(wz + pose[2])};
    counts[so_icp_shard_owner_of_point(q, origin, plane_res, world_size)]++;
  }
  return SO_ICP_OK;
}

}  // extern "C"
