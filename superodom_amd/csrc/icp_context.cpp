// icp_context.cpp -- host driver behind the C ABI of include/so_icp.h.
//
// Mirrors, on top of the HIP kernels, the control flow of
//   LidarSLAM::Localization / performLocalizationAndMapping   src/LidarProcess/LidarSlam.cpp:30-51, 107-210
// (paths relative to /root/reference/super_odometry/).  There is NO CPU fallback: without a usable
// HIP device so_icp_create() fails and says so.
// This file: create / destroy / configuration, the map entries, so_icp_knn_surf, so_icp_register(_dev) and the registration itself
// (register_core), registration_error, the LM entries, timing and debug.  The context and the helpers the driver's translation units
// share: ctx.h.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "ctx.h"

static_assert(sizeof(so_icp_sums) == sizeof(LmSums), "so_icp_sums must mirror LmSums");
static_assert(sizeof(LmState) <= sizeof(so_icp_lm_state), "so_icp_lm_state too small");
static_assert(sizeof(LmSums) == 45 * sizeof(double), "LmSums is 45 doubles");

namespace soicp::host {

thread_local std::string g_create_error;

hipEvent_t next_event(so_icp_ctx* c) {
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->ev_pool.push_back(e);
  }
  return c->ev_pool[c->ev_used++];
}
// time_kernels: 1 = bracket only the dominant (k-NN) kernel -- cheap enough to stay on inside a timed region;
//               2 = bracket every kernel (events cost a few microseconds of pipeline bubble each)
static void span_begin(so_icp_ctx* c, int kind, uint32_t units) {
  if (c->batch_mode || !c->cfg.time_kernels || (c->cfg.time_kernels == 1 && kind != 0)) return;
  EventSpan s{kind, next_event(c), next_event(c), units};
  if (!s.a || !s.b) return;
  (void)hipEventRecord(s.a, c->stream);
  c->spans.push_back(s);
  c->span_open = true;
}
static void span_end(so_icp_ctx* c) {
  if (!c->span_open || c->spans.empty()) return;
  c->span_open = false;
  (void)hipEventRecord(c->spans.back().b, c->stream);
}
static void spans_collect(so_icp_ctx* c) {  // stream must be idle
  for (const EventSpan& s : c->spans) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, s.a, s.b) != hipSuccess) continue;
    if (s.kind == 0) { c->timing.knn_ms_total += ms; c->timing.knn_launches++; c->timing.knn_queries += s.units; c->timing.knn_map_points += c->view.n_points; }
    else if (s.kind == 1) { c->timing.eval_ms_total += ms; c->timing.eval_launches++; c->timing.eval_points += s.units; }
    else { c->timing.prep_ms_total += ms; c->timing.prep_launches++; }
  }
  c->spans.clear();
  c->ev_used = 0;
}

float map_plane_res(const so_icp_ctx* c) { return c->dmap ? c->dmap->plane_res() : c->map.plane_res(); }
void map_shift(so_icp_ctx* c, const double t[3], int pos[3]) { if (c->dmap) c->dmap->shift(t, pos); else c->map.shift(t, pos); }
int map_count_5x5(const so_icp_ctx* c, const int pos[3]) { return c->dmap ? c->dmap->count_5x5(pos) : c->map.count_5x5(pos); }
const int* map_origin(const so_icp_ctx* c) { return c->dmap ? c->dmap->origin() : c->map.origin(); }

int upload_map(so_icp_ctx* c) {
  if (c->dmap) { const int rv = c->dmap->view(c->view, c->err); return map_status(rv); }
  if (c->uploaded_version == c->map.version()) return SO_ICP_OK;
  c->map.build_canonical(c->query_split ? 0 : c->cfg.rank, c->query_split ? 1 : c->cfg.world_size, c->cm);
  const CanonicalMap& m = c->cm;
  const size_t n = m.n_points();
  HIP_TRY(c, c->d_mpts.reserve((n + 16) * 16));
  HIP_TRY(c, c->d_cell_start.reserve((m.cell_start.size() + 1) * 4));
  HIP_TRY(c, c->d_cube_slot.reserve(kMapNum * 4));
  if (n) {
    HIP_TRY(c, hipMemcpyAsync(c->d_mpts.p, m.xyzw.data(), n * 16, hipMemcpyHostToDevice, c->stream));
  }
  if (!m.cell_start.empty())
    HIP_TRY(c, hipMemcpyAsync(c->d_cell_start.p, m.cell_start.data(), m.cell_start.size() * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->d_cube_slot.p, m.cube_slot.data(), kMapNum * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // host vectors may be rebuilt right after
  DevMapView& v = c->view;
  v.pts = c->d_mpts.as<float4>();
  v.cell_start = c->d_cell_start.as<uint32_t>(); v.cube_slot = c->d_cube_slot.as<int32_t>();
  v.nc = m.nc; v.ncell1 = (uint32_t)((size_t)m.nc * m.nc * m.nc + 1); v.inv_cell = 1.0 / m.cell;
  v.origin[0] = c->map.origin()[0]; v.origin[1] = c->map.origin()[1]; v.origin[2] = c->map.origin()[2];
  v.n_points = (uint32_t)n;
  v.n_slots = (uint32_t)m.n_slots;
  c->uploaded_version = c->map.version();
  return SO_ICP_OK;
}

int reserve_scan_buffers(so_icp_ctx* c, size_t n) {
  const size_t m = n + 256;
  HIP_TRY(c, c->d_keys0.reserve(m * 4));
  HIP_TRY(c, c->d_vals0.reserve(m * 4)); HIP_TRY(c, c->d_chunks.reserve(m * 4));
  HIP_TRY(c, c->d_binned.reserve(m * 16));
  HIP_TRY(c, c->d_nd.reserve(m * 32)); HIP_TRY(c, c->d_coeff.reserve(m * 8)); HIP_TRY(c, c->d_status.reserve(m));
  HIP_TRY(c, c->d_nbr5.reserve(m * 20));
  return SO_ICP_OK;
}

MatchParams match_params(float plane_res, int ablate) {
  MatchParams mp;
  mp.plane_res = plane_res;
  mp.sq_max_dist_f = 3 * plane_res;           // float product (LidarSlam.cpp:526)
  mp.max_point_dist = (double)plane_res / 2.0; // LidarSlam.cpp:820
  mp.ablate = ablate;  // SOICP_ABLATE, read when the context is created (a getenv per registration is a walk over environ)
  mp.kdbg = nullptr;
  mp.skip_near_pass = 0;
  mp.pack_light = 1;
  mp.packed_leftover = nullptr;
  mp.begin = 0; mp.begin_max_surface_features = -1; mp.begin_n = 0;
  mp.begin_args = RegBeginArgs{};
  mp.begin_ctr = nullptr; mp.begin_state = nullptr;
  mp.chain_expect = 0;
  return mp;
}
EvalParams eval_params(float plane_res, int variant, int ablate) {
  EvalParams ep;
  const double a = (double)sqrtf(3 * plane_res);  // std::sqrt(float) then TukeyLoss(double a) (LidarSlam.cpp:271)
  ep.a2 = a * a;
  ep.variant = variant;
  ep.ablate = ablate;
  ep.hring[0] = ep.hring[1] = nullptr;
  ep.seq_base = 0;
  ep.n_queries = 0; ep.q_stride = 1;
  ep.defer_publish = 0;
  ep.chain_expect = 0; ep.chain_next = 0;
  for (double& d : ep.chain_delta) d = 0;
  ep.epoch_base = 0;
  for (void*& p : ep.peer_inbox) p = nullptr;
  ep.peer_rank = 0; ep.peer_world = 0;
  ep.timeout_ticks = 5000000ull;  // 50 ms
  return ep;
}
// The parameters of one registration's sweeps and solves (register_core_once and so_icp_register_sequence form them alike: their
// results must be the same bits).  The read-back: the controller's workgroup publishes the state block straight into the pinned
// mirrors `ring`, `ring` + 1 (polled by the host); SOICP_READBACK=copy (or the controller ablated away) leaves them out -- the host
// copies the state block itself.  Returns the registration's report number base.
unsigned long long registration_params(so_icp_ctx* c, float plane_res, size_t n, uint32_t chunk_cap, int ring, MatchParams& mp, EvalParams& ep) {
  mp = match_params(plane_res, c->ablate);
  mp.chunk_cap = chunk_cap;
  mp.pack_light = (c->knn_pack && c->knn_pack_hold == 0 && !c->knn_list_fits) ? 1 : 0;
  mp.packed_leftover = &c->d_state->packed_leftover;
  if (c->knn_pack_hold > 0) --c->knn_pack_hold;
  ep = eval_params(plane_res, c->cfg.tukey_variant, c->ablate);
  const unsigned long long seq_base = (++c->reg_counter) << 8;
  if (c->direct_readback && !(ep.ablate & 32)) { ep.hring[0] = c->d_ring[ring]; ep.hring[1] = c->d_ring[ring + 1]; ep.seq_base = seq_base; }
  ep.n_queries = (uint32_t)n; ep.q_stride = 3;  // evaluation kernels read the scan itself, in its own order
  ep.defer_publish = 0;
  mp.hring[0] = ep.hring[0]; mp.hring[1] = ep.hring[1]; mp.seq_base = ep.seq_base; mp.publish_prev = 0;
  return seq_base;
}
int refuse_scan_size(so_icp_ctx* c) {  // (kernels.hip: bin_offsets_kernel / knn_plane_kernel)
  return fail(c, SO_ICP_E_UNSUPPORTED, "scan of 2^21 points or more: the work-list counters hold 21 bits each (chunk descriptors 26)");
}
// processPlannerFeatures: every kept query in parallel (LidarSlam.cpp:323-344)
void launch_sweep(so_icp_ctx* c, const RegWork& w, MatchParams& mp_it, bool first, const so_icp_ctx::StageSlot* begin_slot, const double pose[7],
                  uint32_t chain_expect, hipEvent_t ev_start, hipEvent_t ev_stop) {
  if (w.query_waves) {
    launch_knn_query_waves(w.d_scan, (uint32_t)w.n, c->d_state, pose, w.max_outer, w.lm_max, first, c->d_hist, c->view, mp_it, c->cfg.max_surface_features,
                           w.corr.status, c->d_nbr5.as<uint32_t>(), c->stream, ev_start, ev_stop, first ? chain_expect : 0u);
  } else {
    if (begin_slot) {  // the first sweep of a scan binned ahead starts the registration itself (MatchParams::begin): the prologue's arguments
      mp_it.begin = 1; mp_it.begin_args.max_outer = w.max_outer; mp_it.begin_args.lm_max = w.lm_max; mp_it.begin_max_surface_features = c->cfg.max_surface_features;
      mp_it.begin_n = (uint32_t)w.n; std::memcpy(mp_it.begin_args.pose, pose, sizeof(mp_it.begin_args.pose));
      mp_it.begin_args.chain_expect = chain_expect; mp_it.begin_args.pad = 0;
      mp_it.begin_ctr = begin_slot->pb_ctr.as<unsigned long long>(); mp_it.begin_state = c->d_state;
    }
    launch_knn_plane(w.d_binned, w.d_chunks, c->d_state, c->view, mp_it, w.corr, c->d_nbr5.as<uint32_t>(), c->d_hist, c->stream, ev_start, ev_stop);
  }
}
// setupOptimizationProblem + solveOptimizationProblem (LidarSlam.cpp:213-240) of one outer iteration: the whole solve in one launch
// (workgroups hand the next pose to each other on the device).  (The span is one of profiling mode, time_kernels 2.)
void launch_persistent_solve(so_icp_ctx* c, const RegWork& w, EvalParams& ep_it, const MatchParams& mp, const PosePrior* prior, bool prior_at_guess) {
  ep_it.epoch_base = (++c->solve_launches) << 5;
  span_begin(c, 1, (uint32_t)w.n);
  launch_solve(w.lm_max, w.d_scan, w.d_scan + 1, w.d_scan + 2, w.corr, c->d_state, ep_it, c->d_partials, c->d_ticket, c->d_hist, c->d_sums, c->view,
               c->d_nbr5.as<uint32_t>(), mp, (uint32_t)w.n, (uint32_t)c->n_cus, c->stream, prior, prior_at_guess);
  span_end(c);
}
Report await_report(so_icp_ctx* c, const volatile unsigned long long* seq, unsigned long long want, hipStream_t s) {
  constexpr int kReportWatchdogMs = 5;  // (a registration lasts 0.15 ms; the waits inside a solve launch give up after 50 ms)
  auto next_check = std::chrono::steady_clock::now() + std::chrono::milliseconds(kReportWatchdogMs);
  for (unsigned spin = 1;; ++spin) {
    if (*seq == want) break;
    if ((spin & 0x3FFu) != 0) continue;
    const auto now = std::chrono::steady_clock::now();
    if (now < next_check) continue;
    next_check = now + std::chrono::milliseconds(1);
    // watchdog: everything enqueued so far -- the launch that reports this iteration included -- has completed
    if (hipStreamQuery(s) != hipErrorNotReady) {
      (void)hipGetLastError();  // (hipErrorNotReady of the earlier polls, or the error the synchronize below reports)
      // the iteration's launches have all completed: either it was a no-op (converged earlier: cannot happen for the
      // iteration the host waits on) or a kernel failed -- report instead of spinning forever
      if (*seq == want) break;
      const hipError_t e = hipStreamSynchronize(s);
      if (e != hipSuccess) { c->err = std::string("hipStreamSynchronize(s): ") + hipGetErrorString(e); return Report::kHipError; }
      if (*seq == want) break;
      return Report::kDrained;
    }
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return Report::kReported;
}
void note_registration_done(so_icp_ctx* c, DevState* mirror, const MatchParams& mp, size_t n, bool sets_list_fits, bool sets_done_count) {
  const DevState& H = *(c->h_state = mirror);
  // the k-NN packing policy (so_icp_ctx::knn_pack_hold)
  if (mp.pack_light) c->timing.knn_pack_registrations++;
  // (the device's count runs on from registration to registration -- nothing on the device clears it beside the sweeps that add to it)
  const uint32_t packed_left = H.packed_leftover >= c->packed_leftover_seen ? H.packed_leftover - c->packed_leftover_seen : H.packed_leftover;
  c->packed_leftover_seen = H.packed_leftover;
  if (mp.pack_light && (double)packed_left > 0.03 * (double)n * (double)std::max(H.n_iterations, 1)) { c->knn_pack_hold = 32; c->timing.knn_pack_holds++; }
  // (scans of a stream have one size: the list of this registration decides the packing of the next -- results do not depend on it;
  //  so_icp_register_sequence leaves it as it is after a registration swept by query waves, which builds no list)
  if (sets_list_fits) c->knn_list_fits = work_list_fits(H.bin_packed, (unsigned long long)kKnnBlocks * 4ull);
  // (registrations completed on the context's own state block, so_icp_register_sequence's chain condition: a batch lane or a
  //  borrowed map leaves the count alone)
  if (sets_done_count) c->done_count_seen = H.done_count;
}

// LidarSLAM::EstimateLidarUncertainty, LidarSlam.cpp:915-964
static void uncertainty_from_hist(const int32_t* H, double u[6]) {
  const double tt = (double)H[6] + H[7] + H[8];
  const double tr = (double)H[0] + H[1] + H[2] + H[3] + H[4] + H[5];
  if (tt == 0 || tr == 0) { for (int i = 0; i < 6; ++i) u[i] = 0; return; }
  u[0] = std::fmin(H[6] / tt * 3, 1.0); u[1] = std::fmin(H[7] / tt * 3, 1.0); u[2] = std::fmin(H[8] / tt * 3, 1.0);
  u[3] = std::fmin((H[0] + H[1]) / tr * 3, 1.0); u[4] = std::fmin((H[2] + H[3]) / tr * 3, 1.0); u[5] = std::fmin((H[4] + H[5]) / tr * 3, 1.0);
}

// LidarSLAM::MannualYawCorrection, LidarSlam.cpp:891-913; tf2::Matrix3x3::getRPY and tf2::Quaternion::setRPY
// [UPSTREAM tf2] written out.
static void yaw_correction(double T[7], const double last[7], double yaw_ratio) {
  double tn, rn;
  relative_motion(last, T, tn, rn);
  const float translation_norm = (float)tn;
  const double x = T[3], y = T[4], z = T[5], w = T[6];
  const double d = x * x + y * y + z * z + w * w, s = 2.0 / d;
  const double xs = x * s, ys = y * s, zs = z * s, wx = w * xs, wy = w * ys, wz = w * zs;
  const double xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
  const double m00 = 1.0 - (yy + zz), m01 = xy - wz, m02 = xz + wy, m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
  double roll, pitch, yaw;
  if (std::fabs(m20) >= 1) {
    yaw = 0;
    const double delta = std::atan2(m01, m02);
    pitch = (m20 < 0) ? M_PI / 2.0 : -M_PI / 2.0;
    roll = delta;
  } else {
    pitch = -std::asin(m20);
    roll = std::atan2(m21 / std::cos(pitch), m22 / std::cos(pitch));
    yaw = std::atan2(m10 / std::cos(pitch), m00 / std::cos(pitch));
  }
  const double cyaw = yaw + translation_norm * yaw_ratio * M_PI / 180;
  const double hy = cyaw * 0.5, hp = pitch * 0.5, hr = roll * 0.5;
  const double cy = std::cos(hy), sy = std::sin(hy), cp = std::cos(hp), sp = std::sin(hp), cr = std::cos(hr), sr = std::sin(hr);
  double q[4] = {sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy};
  const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) T[3 + i] = q[i] / n;
}

// The registration's results out of the state block the device published: pose (LidarSlam.cpp:135-136), per-iteration
// statistics (:242-251), final normal equations, post-processing (:155-157, 198-210).
void fill_result(so_icp_ctx* c, const DevState& H, const double pose_in[7], so_icp_stats* st, double pose_out[7], bool update_tracker) {
  double T[7];
  std::memcpy(T, H.T, sizeof(T));
  st->n_iterations = H.n_iterations;
  for (int it = 0; it < H.n_iterations && it < SO_ICP_MAX_OUTER; ++it) {
    so_icp_iter_stats& is = st->iterations[it];
    const DevIterStats& d = H.iters[it];
    is.translation_norm = d.translation_norm; is.rotation_norm = d.rotation_norm;
    is.num_surf_from_scan = d.num_surf; is.lm_iterations = d.lm_iterations; is.num_successful_steps = d.num_successful;
    is.termination = d.termination; is.initial_cost = d.initial_cost; is.final_cost = d.final_cost;
    std::memcpy(is.reject_hist, d.reject_hist, sizeof(is.reject_hist));
    std::memcpy(is.obs_hist, d.obs_hist, sizeof(is.obs_hist));
    std::memcpy(is.pose_after, d.pose_after, sizeof(is.pose_after));
  }
  if (H.n_iterations > 0 && update_tracker) {
    std::memcpy(c->prev_obs_hist, H.iters[H.n_iterations - 1].obs_hist, sizeof(c->prev_obs_hist));
    c->have_hist = true;
  }
  std::memcpy(st->JtJ, H.JtJ, sizeof(st->JtJ));
  std::memcpy(st->Jtr, H.Jtr, sizeof(st->Jtr));
  yaw_correction(T, pose_in, c->cfg.yaw_ratio);  // performPostOptimizationProcessing, :155-157 (last_T_w_lidar = the guess, :53-57)
  relative_motion(pose_in, T, st->total_translation, st->total_rotation);
  relative_motion(pose_in, T, st->translation_from_last, st->rotation_from_last);
  st->prediction_source = 0;
  std::memcpy(pose_out, T, sizeof(T));
}

void fill_stats_header(const so_icp_ctx* c, so_icp_stats* st, const int pos[3], int count_5x5, size_t n) {
  if (c->have_hist) uncertainty_from_hist(c->prev_obs_hist, st->uncertainty);  // LidarSlam.cpp:47
  st->pos_in_localmap[0] = pos[0]; st->pos_in_localmap[1] = pos[1]; st->pos_in_localmap[2] = pos[2];
  st->laser_cloud_surf_from_map_num = count_5x5; st->laser_cloud_surf_stack_num = (int32_t)n; st->startup_count = c->startup_count;  // LidarSlam.cpp:367
}

namespace {

// One so_icp_register(_dev) registration: every mode of its schedule, resolved once and explained where it is (plan_registration),
// its buffers (claim_buffers) and the parameters of its launches (begin_registration)
struct RegPlan : RegWork {
  const double* pose_in = nullptr;
  size_t n_total = 0;  // the whole scan; n: what this context registers of it (its share under a query split)
  QueryShare share{0, false, 0};
  bool solo = false, qsplit = false, may_prebin = false, begin_in_knn = false, rebin = false, direct_rb = false, timed = false, peer = false,
       exchange = false, persistent = false, defer_reports = false, prior = false;
  so_icp_ctx::StageSlot* pb = nullptr;  // the scan was binned ahead: its work list is in this slot
  uint32_t flags = 0, chunk_cap = 0;    // (flags: what of the modes goes into so_icp_stats::flags)
  BinTable bt{nullptr, nullptr, nullptr, 0};
  MatchParams mp; EvalParams ep;
  unsigned long long seq_base = 0;
  std::vector<size_t> knn_span_of_outer, eval_span_first;  // so_icp_ctx::spans index of every outer iteration's sweep / first evaluation span
};

void plan_registration(const so_icp_ctx* c, RegPlan& p, const float* d_scan, size_t n, const double pose_in[7]) {
  p.d_scan = d_scan; p.n = p.n_total = n; p.pose_in = pose_in;
  p.max_outer = outer_limit(c->cfg.max_iterations);
  p.lm_max = lm_limit(c->cfg.lm_max_iterations);
  // so_icp_match: the matching half of ONE outer iteration and the evaluation at the guess -- lm_begin ends the solve at once
  // (iter >= max_iter, termination 0) with the sums of the guess, and the registration with it (lm_limit maps 0 to 4: not through it)
  if (c->match_only) { p.max_outer = 1; p.lm_max = 0; }
  const bool own = !c->batch_mode && !c->borrow.on;  // this context's own registration, on its own map
  const bool one_device = c->cfg.world_size <= 1;
  const bool controller = !(c->ablate & 32);         // (ablated controller: per-evaluation launches, read-back by copy)
  // SO_ICP_SHARD_QUERIES: this rank registers ITS share of the scan -- the 64-point segments rank, rank + world, ... (a 128-ring
  // sweep in ring-major order gives every rank two 22.5-degree sectors of every ring: spatially compact, so its k-NN chunks are
  // as full as the whole scan's) -- gathered into one array by a strided device copy; from here on the registration is a
  // single-device one over n_own points, except that the sums of every evaluation are exchanged with the other ranks.
  p.qsplit = c->query_split && own;
  if (p.qsplit) { p.share = query_split_share(n, (size_t)c->cfg.world_size, (size_t)c->cfg.rank); p.n = p.share.n_own; }
  p.solo = own && !p.qsplit;
  // A SMALL scan is not binned at all (query_wave_count_ok, reg_plan.h), the prologue rides on the first sweep.  Single device,
  // single registration; the instrumented build keeps the chunked sweep (its stamps describe that kernel).
  p.query_waves = c->query_waves && query_wave_count_ok(c->cfg.max_surface_features, p.n, kQueryWaveMaxKept) && one_device && p.solo && c->ablate == 0;
  // a scan that was binned ahead of this call (so_icp_stage_scan, so_icp_ctx::prebin): its work list is in the slot
  p.may_prebin = c->prebin && c->dmap && one_device && p.solo;
  p.pb = (!p.query_waves && p.may_prebin && p.n && c->scan_staged && c->stage_in_use && c->stage_in_use->prebinned && c->stage_in_use->n == p.n &&
          c->stage_in_use->dev.as<float>() == d_scan) ? c->stage_in_use : nullptr;
  // (the prologue rides on the first k-NN launch -- MatchParams::begin -- unless that is the instrumented instantiation, whose
  //  statistics share the histogram block the prologue clears)
  p.begin_in_knn = p.pb && c->ablate == 0;
  // sharded map: ownership follows the query's cell under the CURRENT pose, so the scan is re-binned at the start of
  // every outer iteration (a 1 degree correction at 50 m moves a point by more than the one-cell halo of a shard)
  p.rebin = !one_device && p.n && !p.qsplit;
  p.direct_rb = c->direct_readback && controller;
  // time_kernels == 1 samples every 3rd registration (a period coprime to the scan rotation of typical benchmarks, so
  // that every scan of the rotation gets timed): even dispatch-attached events cost ~5 us of stream time per
  // timed launch (completion-signal handling), which would otherwise sit inside every step of a throughput run
  p.timed = !c->batch_mode && (c->cfg.time_kernels >= 2 || (c->cfg.time_kernels == 1 && (c->timing.registrations % 3) == 0));
  // (concurrent hypotheses: two persistent launches could each hold part of the CUs and wait for the rest -- one launch per
  //  evaluation there; only workgroup 0 of a launch ever waits, for workgroups that finish unconditionally)
  p.peer = c->peer_on && !one_device && c->persistent_solve && !c->batch_mode && controller;
  p.exchange = !p.peer && (c->comm != nullptr || c->group != nullptr);
  // (so_icp_match: the per-evaluation launch of slot 0, whose one-thread controller is lm_solver.h as it stands; no pass follows it)
  p.persistent = c->persistent_solve && !p.exchange && (!c->batch_mode || c->batch_single) && controller && !c->match_only;
  // deferred report: possible when the host always has the next k-NN launch in the queue before it waits for a report
  p.defer_reports = p.persistent && p.direct_rb && c->speculate;
  // so_icp_set_pose_prior: the PRIOR instantiations of the solve / evaluation kernels add it to every evaluation's sums
  // (a lane of so_icp_register_batch: its hypothesis' prior, armed by the batch itself -- so_icp_set_batch_priors; no public entry
  //  leaves a prior pending on a context in batch mode)
  p.prior = carries_pose_prior(c->pending.kind == kPriorSingle, own || c->batch_mode, c->cfg.world_size, c->match_only) && !p.exchange;
  p.flags = (p.query_waves ? SO_ICP_FLAG_QUERY_WAVES : 0u) | (p.pb ? SO_ICP_FLAG_BINNED_AHEAD : 0u) | (p.persistent ? 0u : SO_ICP_FLAG_PER_EVAL_LAUNCHES) |
            (p.prior ? SO_ICP_FLAG_POSE_PRIOR : 0u);
}

// this rank's share of a split scan gathered into d_sub, the scan buffers, and where the sweeps find their work
int claim_buffers(so_icp_ctx* c, RegPlan& p) {
  if (p.qsplit) {
    const size_t W = (size_t)c->cfg.world_size, r = (size_t)c->cfg.rank, own_full = p.share.own_full, s_full = p.n_total / 64, tail = p.n_total % 64;
    HIP_TRY(c, c->d_sub.reserve((p.n + 64) * 12));
    if (own_full) HIP_TRY(c, hipMemcpy2DAsync(c->d_sub.p, 768, p.d_scan + r * 192, W * 768, 768, own_full, hipMemcpyDeviceToDevice, c->stream));
    if (p.share.own_tail) HIP_TRY(c, hipMemcpyAsync(c->d_sub.as<float>() + own_full * 192, p.d_scan + s_full * 192, tail * 12, hipMemcpyDeviceToDevice, c->stream));
    p.d_scan = c->d_sub.as<float>();
  }
  const int rc = reserve_scan_buffers(c, p.n);
  if (rc) return rc;
  p.d_binned = p.pb ? p.pb->pb_binned.as<float4>() : c->d_binned.as<float4>();
  p.d_chunks = p.pb ? p.pb->pb_chunks.as<uint32_t>() : c->d_chunks.as<uint32_t>();
  p.chunk_cap = p.pb ? p.pb->pb_chunk_cap : (uint32_t)(c->d_chunks.cap / 4);
  p.corr = CorrBuffers{c->d_nd.as<double4>(), c->d_coeff.as<double>(), c->d_status.as<uint8_t>()};
  return SO_ICP_OK;
}

// hash binning: keys + per-key counts (scan_keys), bucket offsets + chunk list (bin_offsets), placement (bin_place).
// The table has >= 2 slots per query; bin_offsets leaves it empty again.  `rebin`: under the CURRENT device-resident pose, no prologue
void launch_hash_binning(so_icp_ctx* c, const RegPlan& p, bool rebin) {
  DevState* ds = c->d_state; hipStream_t s = c->stream;
  launch_scan_keys(p.d_scan, (uint32_t)p.n, ds, p.pose_in, p.max_outer, p.lm_max, c->d_hist, c->view, c->cfg.max_surface_features, c->cfg.rank,
                   c->cfg.world_size, c->d_keys0.as<uint32_t>(), c->d_vals0.as<uint32_t>(), c->d_status.as<uint8_t>(), p.bt, s, rebin, nullptr, 0,
                   p.qsplit, rebin ? 0u : (uint32_t)p.n_total);
  launch_bin_offsets(p.bt, c->d_chunks.as<uint32_t>(), (uint32_t)(c->d_chunks.cap / 4), ds, s);
  launch_bin_place(p.bt, p.d_scan, (uint32_t)p.n, c->d_keys0.as<uint32_t>(), c->d_vals0.as<uint32_t>(), c->d_binned.as<float4>(), s, rebin ? ds : nullptr);
}
// ---- once per registration: prologue (the guess and the loop bounds travel as kernel arguments, no H2D copy),
//      sampling rule, spatial sort (locality survives the small pose updates), chunk list + gather
int begin_registration(so_icp_ctx* c, RegPlan& p) {
  DevState* ds = c->d_state; hipStream_t s = c->stream; const uint32_t n = (uint32_t)p.n;
  span_begin(c, 2, n);
  if (p.query_waves || p.begin_in_knn) {  // (the first sweep starts the registration)
  } else if (p.pb) {
    launch_reg_begin_prebinned(ds, p.pose_in, p.max_outer, p.lm_max, c->d_hist, p.pb->pb_ctr.as<unsigned long long>(), c->d_status.as<uint8_t>(), n,
                               c->cfg.max_surface_features, s);
  } else if (n) {
    const uint32_t lg = bin_table_log2(p.n);
    HIP_TRY(c, c->bin.ensure(lg, s));
    p.bt = c->bin.view();
    c->bin.log2 = 0;  // dirty until bin_offsets has been enqueued behind scan_keys
    launch_hash_binning(c, p, false);
    c->bin.log2 = lg;
  } else {
    launch_scan_keys(p.d_scan, 0, ds, p.pose_in, p.max_outer, p.lm_max, c->d_hist, c->view, c->cfg.max_surface_features, c->cfg.rank,
                     c->cfg.world_size, nullptr, nullptr, nullptr, p.bt, s);  // (empty scan: the prologue alone)
  }
  span_end(c);
  HIP_TRY(c, hipGetLastError());  // a refused launch would otherwise surface as a 50 ms wait or "state was not published"
  // the parameters of the sweeps and solves (host work: it follows the first launches into the queue)
  p.seq_base = registration_params(c, c->borrow.on ? c->borrow.plane_res : map_plane_res(c), p.n, p.chunk_cap, 0, p.mp, p.ep);
  if (p.mp.ablate & 128) {  // profiling: per-workgroup phase stamps of the k-NN sweeps
    HIP_TRY(c, c->d_kdbg.reserve((size_t)2 * kKnnBlocks * 4 * 16 * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemsetAsync(c->d_kdbg.p, 0, (size_t)2 * kKnnBlocks * 4 * 16 * sizeof(unsigned long long), c->stream));
    p.mp.kdbg = c->d_kdbg.as<unsigned long long>();
  }
  if (p.peer) {
    for (int r = 0; r < 8; ++r) p.ep.peer_inbox[r] = c->peer_inbox[r];
    p.ep.peer_rank = c->cfg.rank; p.ep.peer_world = c->cfg.world_size; p.ep.timeout_ticks = c->peer_timeout_ticks;
  }
  p.mp.publish_prev = p.defer_reports ? 1 : 0;
  return SO_ICP_OK;
}

// one evaluation of the per-evaluation schedule: eval(slot) -> (all-reduce -> lm_step)
int enqueue_eval(so_icp_ctx* c, RegPlan& p, int slot) {
  DevState* ds = c->d_state; hipStream_t s = c->stream;
  span_begin(c, 1, (uint32_t)p.n);
  const bool fuse_lm = !p.exchange;  // single device: the last workgroup of eval runs the LM controller itself
  launch_eval(slot, fuse_lm, p.d_scan, p.d_scan + 1, p.d_scan + 2, p.corr, ds, p.ep, c->d_partials,
              c->d_ticket, c->d_hist, c->d_sums, c->view, c->d_nbr5.as<uint32_t>(), p.mp, (uint32_t)p.n, s, p.prior ? &c->pending.single : nullptr);
  span_end(c);
  if (!fuse_lm && c->group) {  // in-process group: through host memory (every member calls this the same number of times)
    HIP_TRY(c, hipMemcpyAsync(c->h_sums, c->d_sums, sizeof(LmSums), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (!group_allreduce(c, c->h_sums))
      return fail(c, SO_ICP_E_RCCL, "in-process group: the exchange of the normal-equation sums failed (a member returned early or did not arrive)");
    HIP_TRY(c, hipMemcpyAsync(c->d_sums, c->h_sums, sizeof(LmSums), hipMemcpyHostToDevice, s));
    launch_lm_step(slot, ds, c->d_sums, c->d_hist, p.ep, s);
  } else if (!fuse_lm) {  // per-evaluation collective: 45 fp64 summed over the shards (xGMI, latency-bound), then the controller
    const ncclResult_t nrc = c->rccl.AllReduce(c->d_sums, c->d_sums, sizeof(LmSums) / sizeof(double), ncclDouble, ncclSum, c->comm, s);
    if (nrc != ncclSuccess) return fail(c, SO_ICP_E_RCCL, std::string("ncclAllReduce: ") + (c->rccl.GetErrorString ? c->rccl.GetErrorString(nrc) : "?"));
    launch_lm_step(slot, ds, c->d_sums, c->d_hist, p.ep, s);
  }
  return SO_ICP_OK;
}

// One outer iteration = knn_plane -> [ eval(slot) -> (all-reduce -> lm_step) ] x (1 + lm_max) -> state read-back.
// (The histogram replicas are cleared by reg_begin and again by the controller when a solve ends:
//  ResetDistanceParameters, LidarSlam.cpp:847-852.)
// part A: correspondences + plane fit + first evaluation; part B: the remaining evaluations + read-back
int enqueue_outer_a(so_icp_ctx* c, RegPlan& p, int it) {
  if (it > 0 && p.rebin) launch_hash_binning(c, p, true);
  p.knn_span_of_outer.push_back(c->spans.size());
  hipEvent_t ka = nullptr, kb = nullptr;
  if (p.timed) {  // the events ride on the dispatch packet (hipExtLaunchKernelGGL), no marker packets
    ka = next_event(c); kb = next_event(c);
    if (ka && kb) c->spans.push_back(EventSpan{0, ka, kb, (uint32_t)p.n});
  }
  MatchParams mp_it = p.mp;
  launch_sweep(c, p, mp_it, it == 0, (it == 0 && p.begin_in_knn) ? p.pb : nullptr, p.pose_in, 0, ka, kb);
  if (c->cfg.time_kernels >= 2)  // kernel statistics of this sweep (profiling mode only)
    HIP_TRY(c, hipMemcpyAsync(c->h_hist + (size_t)it * kHistReplicas * kHistStride, c->d_hist,
                              kHistReplicas * kHistStride * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  // setupOptimizationProblem + solveOptimizationProblem (LidarSlam.cpp:213-240): 1 + lm_max fused evaluations
  p.eval_span_first.push_back(c->spans.size());
  HIP_TRY(c, hipGetLastError());
  if (p.persistent) return SO_ICP_OK;  // the solve launch belongs to part B: only the k-NN sweep is speculated
  return enqueue_eval(c, p, 0);
}
int enqueue_outer_b(so_icp_ctx* c, RegPlan& p, int it) {
  hipStream_t s = c->stream;
  if (p.persistent) {
    EvalParams ep_it = p.ep;
    // (deferred: the k-NN launch of it + 1 will be enqueued before the host waits)
    ep_it.defer_publish = (p.defer_reports && it + 1 < p.max_outer) ? 1 : 0;
    launch_persistent_solve(c, p, ep_it, p.mp, p.prior ? &c->pending.single : nullptr);
  } else {
    for (int slot = 1; slot <= p.lm_max; ++slot) { const int r = enqueue_eval(c, p, slot); if (r) return r; }
  }
  // the whole state block (pose, per-iteration statistics, final normal equations) into this iteration's pinned mirror
  if (!p.direct_rb) HIP_TRY(c, hipMemcpyAsync(c->h_ring[it & 1], c->d_state, sizeof(DevState), hipMemcpyDeviceToHost, s));
  // (a deferred report is complete only after the NEXT k-NN launch: the event is recorded behind that one, see the loop)
  // (the pinned mirrors are polled; the event is the watchdog of that wait only where the stream itself cannot serve as one)
  if (!p.direct_rb) HIP_TRY(c, hipEventRecord(c->ev_outer[it & 1], s));
  HIP_TRY(c, hipGetLastError());
  return SO_ICP_OK;
}
// wait until outer iteration `it` has been reported
int await_outer(so_icp_ctx* c, const RegPlan& p, int it) {
  if (!p.direct_rb) { HIP_TRY(c, hipEventSynchronize(c->ev_outer[it & 1])); return SO_ICP_OK; }
  const Report rep = await_report(c, &c->h_ring[it & 1]->seq, p.seq_base | (unsigned long long)(it + 1), c->stream);
  if (rep != Report::kDrained) return rep == Report::kReported ? SO_ICP_OK : SO_ICP_E_HIP;
  if (p.persistent && p.peer) {
    // The ranks' pass counters (DevState::peer_seq) and inboxes can no longer be assumed equal: chunks of the failed attempt
    // still carry tags the next registration would reuse.  The peer path is left until the caller repeats the collective
    // handshake (so_icp_peer_export clears the inbox and the counter, _connect, _enable).
    c->peer_on = false; c->peer_connected = false;
    return fail(c, SO_ICP_E_HIP, "peer exchange: a solve launch was abandoned (a rank's records did not arrive within SOICP_PEER_TIMEOUT_MS, or the "
                                 "workgroups were not co-resident); the peer exchange is now disabled on this rank until so_icp_peer_export / "
                                 "_connect / _enable are repeated on every rank");
  }
  if (p.persistent) {
    // The persistent solve launch needs all of its workgroups resident at once.  If the device could not provide that
    // (compute units held by another process, a partitioned device, ...) its waits gave up after 50 ms: fall back to
    // one launch per evaluation for the rest of this context's life and run the registration again.
    c->persistent_solve = false;
    c->err = "persistent solve launch did not complete (workgroups not co-resident?): using per-evaluation launches from now on";
    return kRetryWithoutPersistentSolve;
  }
  return fail(c, SO_ICP_E_HIP, "registration state was not published by the device");
}
// the timing events of a timed registration: keep only the launches that did real work (no-op launches after convergence are excluded)
int collect_timing(so_icp_ctx* c, const RegPlan& p, const DevState& H) {
  std::vector<EventSpan> real;
  for (size_t i = 0; i < c->spans.size(); ++i) {
    const EventSpan& sp = c->spans[i];
    bool keep = (sp.kind == 2);
    for (int it = 0; it < H.n_iterations && !keep; ++it) {
      if (sp.kind == 0 && it < (int)p.knn_span_of_outer.size() && i == p.knn_span_of_outer[it]) keep = true;
      // (a persistent solve launch is ONE span per outer iteration, the per-evaluation schedule 1 + #LM iterations)
      if (sp.kind == 1 && it < (int)p.eval_span_first.size() && i >= p.eval_span_first[it] &&
          i < p.eval_span_first[it] + (p.persistent ? 1 : 1 + (size_t)std::max(H.iters[it].lm_iterations, 0))) keep = true;
    }
    if (keep) { EventSpan r = sp; r.units = work_list_kept(H.bin_packed); real.push_back(r); }
  }
  c->spans.swap(real);
  // profiling mode brackets the solve launches too: the last one has published its result but its stop event may not
  // have signalled yet (hipEventElapsedTime would refuse it) -- wait for the stream there; the k-NN events of mode 1
  // completed long ago
  if (c->cfg.time_kernels >= 2) HIP_TRY(c, hipStreamSynchronize(c->stream));
  spans_collect(c);
  for (int it = 0; it < H.n_iterations && c->cfg.time_kernels >= 2; ++it)
    for (int r = 0; r < kHistReplicas; ++r) {
      const int32_t* hh = c->h_hist + ((size_t)it * kHistReplicas + r) * kHistStride;
      c->timing.knn_group_passes += hh[16]; c->timing.knn_fallback_lanes += hh[17];
      c->timing.knn_packed_rows += hh[20]; c->timing.knn_packed_rows_too_many_runs += hh[21]; c->timing.knn_packed_rows_tile_full += hh[22];
      c->timing.knn_packed_kept += hh[23];
      c->timing.knn_candidates_scanned += (int64_t)hh[18] * 16;
    }
  return SO_ICP_OK;
}

}  // namespace

// LidarSLAM::performLocalizationAndMapping (LidarSlam.cpp:107-152) with the loop state resident on the device:
// the host enqueues, per outer iteration, the STATIC sequence
//     clear histograms -> knn_plane -> [ eval(slot) -> (all-reduce) -> lm_step(slot) ] x (1 + lm_max)
// and every kernel consults DevState (reg_done / lm_more) to turn itself into a no-op once the controller has
// finished -- no host round trip per evaluation.  One small read-back per outer iteration tells the host when to stop
// enqueuing.
static int register_core_once(so_icp_ctx* c, const float* d_scan, size_t n, const double pose_in[7], double pose_out[7], so_icp_stats* st) {
  const auto t_begin = std::chrono::steady_clock::now();
  so_icp_stats local;
  if (!st) st = &local;
  std::memset(st, 0, sizeof(*st));
  if (n >= kMaxScanPoints) return refuse_scan_size(c);
  const bool keep_corr = keeps_correspondences(c);  // so_icp_keep_correspondences: this registration leaves its set for so_icp_correspondences
  if (!c->batch_mode && !c->borrow.on) c->corr_last.valid = false;
  st->flags = (c->retried ? SO_ICP_FLAG_RETRIED : 0u) | (!c->dmap && !c->borrow.on ? SO_ICP_FLAG_HOST_MAP : 0u) |
              (c->cfg.world_size > 1 ? SO_ICP_FLAG_SHARDED : 0u) | (c->query_split ? SO_ICP_FLAG_QUERY_SPLIT : 0u) |
              (c->scan_staged ? SO_ICP_FLAG_STAGED_SCAN : 0u) | (c->direct_readback ? 0u : SO_ICP_FLAG_COPY_READBACK);
  std::memcpy(pose_out, pose_in, 7 * sizeof(double));  // LidarSlam.cpp:53-57 (T_w_initial_guess = last_T_w_lidar = T_w_lidar = the guess)
  int pos[3];
  if (c->borrow.on) std::memcpy(pos, c->borrow.pos, sizeof(pos));  // window, count and map view were fixed by the batch driver
  else if (!c->no_map_shift && !c->no_map_shift_once) { map_shift(c, pose_in, pos); std::memcpy(c->last_pos, pos, sizeof(pos)); }  // LidarSlam.cpp:363
  else std::memcpy(pos, c->last_pos, sizeof(pos));
  c->no_map_shift_once = false;
  fill_stats_header(c, st, pos, c->borrow.on ? c->borrow.count_5x5 : map_count_5x5(c, pos), n);
  if (!(st->laser_cloud_surf_from_map_num > 50)) return SO_ICP_NOT_ENOUGH_MAP_FEATURES;  // LidarSlam.cpp:113-116
  int rc = SO_ICP_OK;
  if (c->borrow.on) c->view = c->borrow.view; else rc = upload_map(c);
  if (rc) return rc;
  RegPlan p;
  plan_registration(c, p, d_scan, n, pose_in);
  if ((rc = claim_buffers(c, p))) return rc;
  // (the scan may lie in a stage slot that is refilled once this call has returned: the copy goes in front of the first launch, so it
  //  has been made when the registration reports)
  if (keep_corr && (rc = keep_scan_copy(c, p.d_scan, p.n))) return rc;
  const auto t_icp = std::chrono::steady_clock::now();  // TicToc t_opt, LidarSlam.cpp:118
  if ((rc = begin_registration(c, p))) return rc;
  st->flags |= p.flags;
  // The host stays ahead of what it knows: part A of iteration it+1 (the k-NN sweep; with a sharded map also the fit
  // evaluation) is enqueued before the report of iteration it is awaited, so the device never idles on a host round trip;
  // part B (the solve launch / the remaining evaluations) follows as soon as the report says "not converged" -- the device
  // is then busy with part A for tens of microseconds.  If iteration it did converge, the speculated launch is a no-op
  // (every kernel consults DevState::reg_done) that drains while the host post-processes.
  // (SOICP_SPECULATE=0 enqueues nothing ahead: every launch of a profiled run is then a real one.)
  int last = 0;
  if ((rc = enqueue_outer_a(c, p, 0))) return rc;
  // the NEXT scan's DMA goes out right behind this registration's first launch (the rest of what the copy queue does for that
  // scan follows below, once the launches that are not urgent -- the first sweep lasts 20 us -- are in the queue as well)
  if (!c->batch_mode && !c->match_only) stage_issue_deferred_copy(c);  // (so_icp_match leaves announced scans where they are)
  if ((rc = enqueue_outer_b(c, p, 0))) return rc;
  for (int it = 0;; ++it) {
    if (c->speculate && it + 1 < p.max_outer && (rc = enqueue_outer_a(c, p, it + 1))) return rc;
    // this registration's launches are in the queue and the host is about to idle: the moment for the NEXT scan's DMA
    if (!c->batch_mode && !c->match_only && it == 0) {
      stage_issue_deferred(c, (p.may_prebin && !p.query_waves) ? pose_in : nullptr);  // (the next scan is binned behind its copy, under this registration's guess; a stream of small scans is not binned at all)
    }
    if ((rc = await_outer(c, p, it))) return rc;
    last = it;
    if (c->h_ring[it & 1]->reg_done || it + 1 >= p.max_outer) break;
    if (!c->speculate && (rc = enqueue_outer_a(c, p, it + 1))) return rc;  // SOICP_SPECULATE=0: no launch that could turn out a no-op
    if ((rc = enqueue_outer_b(c, p, it + 1))) return rc;
  }
  note_registration_done(c, c->h_ring[last & 1], p.mp, p.n, !c->match_only, !c->batch_mode && !c->borrow.on);
  const DevState& H = *c->h_state;
  fill_result(c, H, pose_in, st, pose_out, !c->batch_mode && !c->match_only);
  if (p.prior) st->prediction_source = 1;  // addAbsolutePoseConstraints, LidarSlam.cpp:297
  if (keep_corr) note_correspondences(c, H, pose_in, p.n, p.ep);
  if (c->seq_corr_frame >= 0 && (rc = seq_corr_note_plain(c, p.d_scan, p.n, H, pose_in, p.ep))) return rc;  // (a frame of a run that keeps its sets)
  if (keep_corr && keeps_correspondence_geometry(c)) {  // (the report is in: d_status and d_nbr5 are the last fit pass's; the caller's insert comes behind)
    if ((rc = keep_neighbour_snapshot(c, p.n))) return rc;
    note_correspondence_geometry(c, p.mp);
  }
  st->time_elapsed_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_icp).count();  // :199-200
  if (p.timed && (rc = collect_timing(c, p, H))) return rc;
  if (c->match_only) return SO_ICP_OK;  // (not a registration of so_icp_timing)
  c->timing.registrations++;
  c->timing.host_ms_total += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  return SO_ICP_OK;
}

int register_core(so_icp_ctx* c, const float* d_scan, size_t n, const double pose_in[7], double pose_out[7], so_icp_stats* st) {
  int rc = register_core_once(c, d_scan, n, pose_in, pose_out, st);
  if (rc == kRetryWithoutPersistentSolve) {
    c->no_map_shift_once = true;  // the window was already placed for this scan
    c->retried = true;            // so_icp_stats::flags tells the caller (the context stays on per-evaluation launches)
    rc = register_core_once(c, d_scan, n, pose_in, pose_out, st);
    c->retried = false;
    if (rc == kRetryWithoutPersistentSolve) rc = fail(c, SO_ICP_E_HIP, "registration state was not published by the device");
  }
  // The other members of an in-process group must not wait for this one's next exchange -- when this one FAILED MID-SEQUENCE (a
  // device or exchange error).  A call refused on its arguments (scan too large, bad stride: checked before anything is
  // enqueued or exchanged, and refused alike on every member, which all pass the same scan) leaves the group usable.
  if (rc == SO_ICP_E_HIP || rc == SO_ICP_E_RCCL) group_abort(c);
  return rc;
}

// wait = false: the caller enqueues the scan's consumers on the same stream and does not return to ITS caller before they
// have completed (so_icp_register), so the source buffer outlives the copy without a host-side wait here
// The queue of the host-in / host-out steps around Localization() (pre-filter, de-skew, registered scan): they touch nothing the
// map insert of the previous frame uses, so they need not wait behind it in the context's queue.
hipStream_t aux_stream(so_icp_ctx* c) {
  std::lock_guard<std::mutex> lk(c->aux_mu);  // (created on first use, and so_icp_prefilter_announce may be that use, on the callback's thread)
  if (!c->pf_stream && hipStreamCreateWithFlags(&c->pf_stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); return c->stream; }
  return c->pf_stream;
}

int upload_scan_impl(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, DevBuf& dst, bool wait) {
  if (const int rc = normalise_stride(c, &stride_bytes)) return rc;
  HIP_TRY(c, dst.reserve((n + 64) * 12));
  if (!n) return SO_ICP_OK;
  if (stride_bytes == 12) {
    // The map insert of the previous Localization() may still be in the context's queue: the upload then goes through the
    // auxiliary queue, beside it, and the context's queue waits for the copy's event (nothing in flight reads `dst`: the
    // registration that used it has reported, the insert's only reader of it finished before that call returned).
    hipStream_t s2 = (!wait && c->dmap && c->dmap->insert_in_flight()) ? aux_stream(c) : c->stream;
    if (s2 != c->stream && !c->ev_upload && hipEventCreateWithFlags(&c->ev_upload, hipEventDisableTiming) != hipSuccess) { (void)hipGetLastError(); s2 = c->stream; }
    HIP_TRY(c, hipMemcpyAsync(dst.p, xyz, n * 12, hipMemcpyHostToDevice, s2));
    if (s2 != c->stream) { HIP_TRY(c, hipEventRecord(c->ev_upload, s2)); HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_upload, 0)); }
    if (wait) HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    std::vector<float> packed(n * 3);
    const size_t sf = stride_bytes / 4;
    for (size_t i = 0; i < n; ++i) { packed[3 * i] = xyz[i * sf]; packed[3 * i + 1] = xyz[i * sf + 1]; packed[3 * i + 2] = xyz[i * sf + 2]; }
    HIP_TRY(c, hipMemcpyAsync(dst.p, packed.data(), n * 12, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return SO_ICP_OK;
}

}  // namespace soicp::host

so_icp_ctx::~so_icp_ctx() {
  if (group) group_leave(this);
  if (stage_started) {
    { std::lock_guard<std::mutex> lk(stage_mu); stage_quit = true; }
    stage_pending.fetch_add(1);
    stage_cv.notify_all();
    if (stage_thread.joinable()) stage_thread.join();
  }
  if (copy_stream) (void)hipStreamSynchronize(copy_stream);
  if (seq_stream) (void)hipStreamSynchronize(seq_stream);
  if (fe_state) { if (pf_stream) (void)hipStreamSynchronize(pf_stream); if (stream) (void)hipStreamSynchronize(stream); fe_state.reset(); }
  for (StageSlot& sl : seq_slot) sl.release();
  sbin.release();
  if (seq_stream) (void)hipStreamDestroy(seq_stream);
  for (StageSlot& sl : stage) sl.release();
  for (const HostRange& r : host_ranges) { if (r.owned) (void)hipHostFree(const_cast<char*>(r.p)); else (void)hipHostUnregister(const_cast<char*>(r.p)); }
  for (int r = 0; r < 8; ++r) if (peer_opened[r] && peer_inbox[r]) (void)hipIpcCloseMemHandle(peer_inbox[r]);
  if (peer_own) (void)hipFree(peer_own);
  if (copy_stream) (void)hipStreamDestroy(copy_stream);
  for (so_icp_ctx* w : workers) delete w;
  batch.release();
  if (comm && rccl.CommDestroy) rccl.CommDestroy(comm);
  for (DevBuf* b : {&d_world, &d_mpts, &d_cell_start, &d_cube_slot, &d_scan_own, &d_keys0, &d_vals0, &d_chunks,
                    &d_binned, &d_nd, &d_coeff, &d_status, &d_nbr5, &corr_scan, &d_small, &d_q, &d_nbr, &d_d2, &d_idx,
                    &d_found, &d_fblist, &d_kdbg, &pf_stage, &pf_in, &pf_out, &pf_small, &pf_w, &pf_s, &pf_k0, &pf_k1, &pf_v0, &pf_v1, &pf_flags, &pf_pos,
                    &pf_heads, &pf_temp, &pf_dec, &d_counts, &d_sub, &d_inten, &pf_inten})
    b->release();
  bin.release(); pbin.release();
  for (DevBuf& b : resident_scans) b.release();
  d_state_buf.release();
  for (DevState* h : h_ring) if (h) (void)hipHostFree(h);
  for (hipEvent_t e : ev_outer) if (e) (void)hipEventDestroy(e);
  if (h_hist) (void)hipHostFree(h_hist);
  if (h_sums) (void)hipHostFree(h_sums);
  if (h_u32) (void)hipHostFree(h_u32);
  if (h_pf) (void)hipHostFree(h_pf);
  if (h_pf_kept) (void)hipHostFree(h_pf_kept);
  if (h_inten) (void)hipHostFree(h_inten);
  for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
  dmap.reset();  // (waits for a deferred insert on `stream`)
  if (pf_stream) { (void)hipStreamSynchronize(pf_stream); (void)hipStreamDestroy(pf_stream); }
  if (ev_upload) (void)hipEventDestroy(ev_upload);
  if (stream) (void)hipStreamDestroy(stream);
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int so_icp_abi_version(void) { return SO_ICP_ABI_VERSION; }

void so_icp_default_config(so_icp_config* cfg) {
  if (!cfg) return;
  std::memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = SO_ICP_ABI_VERSION;
  cfg->device_id = 0; cfg->rank = 0; cfg->world_size = 1;
  cfg->max_iterations = 5;          // config/os1_128.yaml:27 (code default 4, LidarSlam.h:273)
  cfg->lm_max_iterations = 4;       // LidarSlam.cpp:232
  cfg->max_surface_features = 2000; // config/os1_128.yaml:28
  cfg->k = 5;                       // LidarSlam.h:277
  cfg->tukey_variant = 0;
  cfg->time_kernels = 0;
  cfg->line_res = 0.1f; cfg->plane_res = 0.2f;  // config/os1_128.yaml mapping_{line,plane}_resolution
  cfg->yaw_ratio = 0.0;
  cfg->velocity_failure_threshold = 30.0;
}

int so_icp_device_available(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

int so_icp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}

const char* so_icp_last_error(const so_icp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

so_icp_ctx* so_icp_create(const so_icp_config* cfg) {
  g_create_error.clear();
  if (!cfg || cfg->abi_version != SO_ICP_ABI_VERSION) { g_create_error = "so_icp_create: bad config / ABI version"; return nullptr; }
  if (cfg->k != 5) { g_create_error = "so_icp_create: only k = 5 (LocalizationPlaneDistanceNbrNeighbors) is supported"; return nullptr; }
  if (cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size) { g_create_error = "so_icp_create: bad rank/world_size"; return nullptr; }
  if (cfg->device_id < 0) {  // host-only: map bookkeeping for tools/tests; compute calls return SO_ICP_E_HIP
    so_icp_ctx* h = new (std::nothrow) so_icp_ctx();
    if (!h) { g_create_error = "out of memory"; return nullptr; }
    h->cfg = *cfg; h->host_only = true;
    h->map.set_resolution(cfg->line_res, cfg->plane_res);
    return h;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_create_error = "so_icp_create: no HIP device available (libsoicp has no CPU fallback)";
    return nullptr;
  }
  if (cfg->device_id < 0 || cfg->device_id >= ndev) { g_create_error = "so_icp_create: device_id out of range"; return nullptr; }
  if ((e = hipSetDevice(cfg->device_id)) != hipSuccess) { g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e); return nullptr; }
  so_icp_ctx* c = new (std::nothrow) so_icp_ctx();
  if (!c) { g_create_error = "out of memory"; return nullptr; }
  c->cfg = *cfg;
  c->map.set_resolution(cfg->line_res, cfg->plane_res);
  auto bail = [&](const std::string& m) { g_create_error = m; delete c; return (so_icp_ctx*)nullptr; };
  if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess) return bail(std::string("hipStreamCreate: ") + hipGetErrorString(e));
  {  // the persistent solve launch holds one workgroup per compute unit: never ask for more than the device has
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, cfg->device_id) == hipSuccess && cus > 0) c->n_cus = cus;
    if (cfg->solve_workgroups >= 1 && cfg->solve_workgroups < c->n_cus) c->n_cus = cfg->solve_workgroups;  // leave compute units to others
    if (const char* ev = std::getenv("SOICP_SOLVE_WORKGROUPS")) { const int w = std::atoi(ev); if (w >= 1 && w < c->n_cus) c->n_cus = w; }
  }
  const size_t partial_bytes = std::max((size_t)kFitBlocksMax * kSumsStride * sizeof(double),
                                        (size_t)kFitBlocksMax * kRecordChunksMax * 16);  // partial sums / tagged records of solve_kernel
  const size_t small_bytes = 4096 + sizeof(LmSums) + 256 + partial_bytes + 256 + kSyncBytes;
  if ((e = c->d_small.reserve(small_bytes)) != hipSuccess) return bail(std::string("hipMalloc: ") + hipGetErrorString(e));
  if ((e = hipMemset(c->d_small.p, 0, c->d_small.cap)) != hipSuccess) return bail(std::string("hipMemset: ") + hipGetErrorString(e));
  char* base = c->d_small.as<char>();
  c->d_hist = reinterpret_cast<int32_t*>(base);            // kHistReplicas x kHistStride ints (2 KB)
  c->d_nkept = reinterpret_cast<uint32_t*>(base + 2112);   // Seam B scratch counters
  c->d_fbcount = reinterpret_cast<uint32_t*>(base + 2176);
  c->d_sums = reinterpret_cast<LmSums*>(base + 4096);
  c->d_partials = reinterpret_cast<double*>(base + 4096 + ((sizeof(LmSums) + 255) / 256) * 256);
  c->d_ticket = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(c->d_partials) + ((partial_bytes + 255) / 256) * 256);  // arrival counters + hand-off record (kSyncBytes)
  if ((e = hipHostMalloc(reinterpret_cast<void**>(&c->h_sums), sizeof(LmSums))) != hipSuccess) return bail(std::string("hipHostMalloc: ") + hipGetErrorString(e));
  if ((e = hipHostMalloc(reinterpret_cast<void**>(&c->h_u32), 64)) != hipSuccess) return bail(std::string("hipHostMalloc: ") + hipGetErrorString(e));
  if ((e = c->d_state_buf.reserve(sizeof(DevState))) != hipSuccess) return bail(std::string("hipMalloc: ") + hipGetErrorString(e));
  if ((e = hipMemset(c->d_state_buf.p, 0, sizeof(DevState))) != hipSuccess) return bail(std::string("hipMemset: ") + hipGetErrorString(e));
  c->d_state = c->d_state_buf.as<DevState>();
  for (int i = 0; i < 4; ++i) {
    if ((e = hipHostMalloc(reinterpret_cast<void**>(&c->h_ring[i]), sizeof(DevState), hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess)
      return bail(std::string("hipHostMalloc: ") + hipGetErrorString(e));
    std::memset(c->h_ring[i], 0, sizeof(DevState));
    if ((e = hipHostGetDevicePointer(reinterpret_cast<void**>(&c->d_ring[i]), c->h_ring[i], 0)) != hipSuccess) return bail(std::string("hipHostGetDevicePointer: ") + hipGetErrorString(e));
    if (i < 2 && (e = hipEventCreateWithFlags(&c->ev_outer[i], hipEventDisableTiming)) != hipSuccess) return bail(std::string("hipEventCreate: ") + hipGetErrorString(e));
  }
  c->h_state = c->h_ring[0];
  if ((e = hipHostMalloc(reinterpret_cast<void**>(&c->h_hist), (size_t)SO_ICP_MAX_OUTER * kHistReplicas * kHistStride * sizeof(int32_t))) != hipSuccess)
    return bail(std::string("hipHostMalloc: ") + hipGetErrorString(e));
  if (const char* ev = std::getenv("SOICP_READBACK")) c->direct_readback = std::string(ev) != "copy";
  if (const char* ev = std::getenv("SOICP_SPECULATE")) c->speculate = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_PREFILTER_FAST")) c->pf_fast = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_ABLATE")) c->ablate = std::atoi(ev);
  if (const char* ev = std::getenv("SOICP_PEER_TIMEOUT_MS")) { const long ms = std::atol(ev); if (ms >= 1 && ms <= 60000) c->peer_timeout_ticks = (unsigned long long)ms * 100000ull; }
  if (const char* ev = std::getenv("SOICP_PERSISTENT")) c->persistent_solve = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_KNN_PACK")) c->knn_pack = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_QUERY_WAVES")) c->query_waves = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_PREBIN")) c->prebin = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_SEQ_CHAIN")) c->seq_chain = std::atoi(ev) != 0;
  if (const char* ev = std::getenv("SOICP_BATCH_CHAIN")) c->batch_chain = std::string(ev) != "0";
  if (const char* ev = std::getenv("SOICP_BATCH_MODE")) {  // "one_per_cu": one solve workgroup per compute unit (several processes on one device); "lanes"
    if (std::string(ev) == "one_per_cu") c->batch_degrade = 1;
    if (std::string(ev) == "lanes") c->batch_degrade = 2;
  }
  const bool want_dmap = !(std::getenv("SOICP_HOST_MAP") && std::atoi(std::getenv("SOICP_HOST_MAP")));
  if (want_dmap) {  // world_size > 1: this rank's shard of the map, resident and updated on the device like the whole map is
    c->query_split = cfg->world_size > 1 && cfg->shard_mode == SO_ICP_SHARD_QUERIES;
    if (c->query_split) c->dmap = std::make_unique<DeviceMap>(c->stream, 0, 1);  // the whole map on every rank
    else c->dmap = std::make_unique<DeviceMap>(c->stream, cfg->rank, cfg->world_size);
    if (!c->dmap->supported_resolution(cfg->plane_res)) c->dmap.reset();  // leaf keys hold 9 bits per axis
    else { std::string e2; c->dmap->set_resolution(cfg->line_res, cfg->plane_res, e2); }
  }
  return c;
}

void so_icp_destroy(so_icp_ctx* ctx) {
  if (!ctx) return;
  if (ctx->host_only) { delete ctx; return; }
  (void)hipSetDevice(ctx->cfg.device_id);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  delete ctx;
}

int so_icp_set_resolution(so_icp_ctx* c, float line_res, float plane_res) {
  if (!c || !(plane_res > 0) || !(line_res > 0)) return SO_ICP_E_INVALID;
  if (c->dmap && !c->dmap->supported_resolution(plane_res)) return fail(c, SO_ICP_E_UNSUPPORTED, "device map needs plane_res >= 0.05 (leaf coordinates of the grouping keys hold 10 bits)");
  // ("non-empty" must be the same decision on every rank: the FULL map's count, which the ranks share after any insert under the
  //  communicator -- a rank whose own shard happens to be empty still takes part in the exchange)
  if (c->dmap && c->dmap->sharded() && c->cfg.world_size > 1 && plane_res != map_plane_res(c) &&
      ((c->group || c->comm) ? c->dmap->size() : c->dmap->size_local()) > 0) {
    // A shard holds the leaves within one CELL of the bricks it owns, and cell size and bricks follow planeRes: after a
    // change the resident subset would no longer cover the gate balls of the rank's queries (wrong neighbours, silently).
    // The shards are re-cut from every rank's points -- a collective step; without a communicator it cannot be done.
    NEED_DEVICE(c);
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    if (!c->group && !c->comm)
      return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_resolution: planeRes cannot change under a sharded, non-empty map without a communicator "
                                            "(the shards are cut along the cell grid that follows planeRes; re-cutting them needs the other ranks' points)");
    const int rc = reshard_for_resolution(c, line_res, plane_res);
    if (rc) return rc;
    c->map.set_resolution(line_res, plane_res);
    c->cfg.line_res = line_res; c->cfg.plane_res = plane_res;
    return SO_ICP_OK;
  }
  if (c->dmap) {
    NEED_DEVICE(c);
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    if (c->dmap->set_resolution(line_res, plane_res, c->err) < 0) return SO_ICP_E_HIP;
  }
  if (plane_res != c->map.plane_res()) c->uploaded_version = 0;  // cell size follows planeRes
  c->map.set_resolution(line_res, plane_res);
  c->cfg.line_res = line_res; c->cfg.plane_res = plane_res;
  return SO_ICP_OK;
}
// The surf cloud's fourth field (pcl::PointXYZI::intensity) through pre-filter, insert and export -- so_icp.h has the rules
int so_icp_set_cloud_intensity(so_icp_ctx* c, int offset_bytes) {
  if (!c) return SO_ICP_E_INVALID;
  if (offset_bytes == -1) { c->intensity_off = -1; return SO_ICP_OK; }
  if (offset_bytes < 12 || offset_bytes % 4) return fail(c, SO_ICP_E_INVALID, "so_icp_set_cloud_intensity: -1, or the 4-byte aligned offset (>= 12) of a FLOAT32 behind x y z");
  if (c->host_only) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_cloud_intensity: a host-only context keeps no intensity");
  if (!c->dmap) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_cloud_intensity: the host-side map (SOICP_HOST_MAP=1, plane_res < 0.05) keeps no intensity");
  if (c->cfg.world_size > 1) return fail(c, SO_ICP_E_UNSUPPORTED, "so_icp_set_cloud_intensity: sharded maps (world_size > 1) keep no intensity");
  c->intensity_off = offset_bytes;
  return SO_ICP_OK;
}
int so_icp_set_max_surface_features(so_icp_ctx* c, int v) { if (!c) return SO_ICP_E_INVALID; c->cfg.max_surface_features = v; return SO_ICP_OK; }
int so_icp_set_max_iterations(so_icp_ctx* c, int v) { if (!c || v < 1) return SO_ICP_E_INVALID; c->cfg.max_iterations = v; return SO_ICP_OK; }

int so_icp_map_set_origin(so_icp_ctx* c, const double t[3], int o[3]) {
  if (!c || !t) return SO_ICP_E_INVALID;
  if (c->dmap) c->dmap->set_origin(t); else c->map.set_origin(t);
  if (o) { o[0] = map_origin(c)[0]; o[1] = map_origin(c)[1]; o[2] = map_origin(c)[2]; }
  return SO_ICP_OK;
}
int so_icp_map_get_origin(so_icp_ctx* c, int o[3]) {
  if (!c || !o) return SO_ICP_E_INVALID;
  o[0] = map_origin(c)[0]; o[1] = map_origin(c)[1]; o[2] = map_origin(c)[2];
  return SO_ICP_OK;
}
int so_icp_map_shift(so_icp_ctx* c, const double t[3], int pos[3]) {
  if (!c || !t || !pos) return SO_ICP_E_INVALID;
  map_shift(c, t, pos);
  return SO_ICP_OK;
}
int so_icp_map_add_surf(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes) {
  if (!c || (!xyz && n)) return SO_ICP_E_INVALID;
  if (const int rc = normalise_stride(c, &stride_bytes)) return rc;
  if (c->dmap) {  // bin + VoxelGrid + index rebuild on the device (map_kernels.hip)
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    const int r = c->dmap->add_surf_host(xyz, n, stride_bytes / 4, c->err, intensity_in(c, xyz, stride_bytes), stride_bytes / 4);
    if (r < 0) { group_abort(c); return map_status(r); }
    const int xr = exchange_map_counts(c);
    return xr ? xr : r;
  }
  return c->map.add_surf(xyz, n, stride_bytes / 4);
}
int so_icp_map_count_5x5(so_icp_ctx* c, const int pos[3], int* n_edge, int* n_surf) {
  if (!c || !pos) return SO_ICP_E_INVALID;
  if (n_edge) *n_edge = 0;
  if (n_surf) *n_surf = map_count_5x5(c, pos);
  return SO_ICP_OK;
}
int so_icp_map_export(so_icp_ctx* c, float* xyz, size_t cap, size_t* n_out, int only_5x5, const int pos[3]) {
  if (!c || (only_5x5 && !pos)) return SO_ICP_E_INVALID;
  const int zero[3] = {0, 0, 0};
  if (c->dmap) HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  const size_t n = c->dmap ? c->dmap->export_points(xyz, cap, only_5x5 != 0, pos ? pos : zero, c->err)
                           : c->map.export_points(xyz, cap, only_5x5 != 0, pos ? pos : zero);
  if (n_out) *n_out = n;
  return SO_ICP_OK;
}
int so_icp_map_export_records(so_icp_ctx* c, void* out, size_t stride_bytes, size_t cap, size_t* n_out, int only_5x5, const int pos[3]) {
  if (!c || (only_5x5 && !pos)) return SO_ICP_E_INVALID;
  if (stride_bytes < 12 || stride_bytes % 4) return fail(c, SO_ICP_E_INVALID, "records: float x y z at 0 4 8, stride a multiple of 4");
  const int zero[3] = {0, 0, 0};
  size_t n = 0;
  if (c->dmap) {
    HIP_TRY(c, hipSetDevice(c->cfg.device_id));
    c->err.clear();
    n = c->dmap->export_records(out, stride_bytes, cap, only_5x5 != 0, pos ? pos : zero, c->intensity_off >= 0, c->err);
    if (!c->err.empty()) return SO_ICP_E_HIP;
  } else {  // host-side map (sharded ranks, host-only contexts): through the packed export
    n = c->map.export_points(nullptr, 0, only_5x5 != 0, pos ? pos : zero);
    if (out && n <= cap && n) {
      std::vector<float> xyz(3 * n);
      c->map.export_points(xyz.data(), n, only_5x5 != 0, pos ? pos : zero);
      std::memset(out, 0, n * stride_bytes);
      for (size_t i = 0; i < n; ++i) std::memcpy(static_cast<char*>(out) + i * stride_bytes, &xyz[3 * i], 12);
    }
  }
  if (n_out) *n_out = n;
  return SO_ICP_OK;
}
int so_icp_map_size(so_icp_ctx* c, size_t* n, size_t* n_rank) {
  if (!c) return SO_ICP_E_INVALID;
  if (n) *n = c->dmap ? c->dmap->size() : c->map.size();
  if (n_rank) { NEED_DEVICE(c); const int rc = upload_map(c); if (rc) return rc; *n_rank = c->view.n_points; }
  return SO_ICP_OK;
}
int so_icp_map_insert_stats(so_icp_ctx* c, unsigned* device_built, unsigned* handed_back) {
  if (!c) return SO_ICP_E_INVALID;
  unsigned a = 0, b = 0;
  if (c->dmap) { std::string e; (void)c->dmap->settle(e); c->dmap->fast_stats(a, b); }
  if (device_built) *device_built = a;
  if (handed_back) *handed_back = b;
  return SO_ICP_OK;
}
int so_icp_map_clear(so_icp_ctx* c) { if (!c) return SO_ICP_E_INVALID; if (c->dmap) c->dmap->clear(); else c->map.clear(); return SO_ICP_OK; }

int so_icp_knn_surf(so_icp_ctx* c, const float* q, size_t nq, int k, float* nbr, float* d2, int32_t* idx, uint8_t* found) {
  if (!c || (!q && nq) || !nbr || !d2 || !found) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (k < 1 || k > 5) return fail(c, SO_ICP_E_UNSUPPORTED, "k must be in [1,5]");
  if (c->cfg.world_size != 1) return fail(c, SO_ICP_E_UNSUPPORTED, "Seam B needs the whole map on one device (world_size == 1)");
  if (!nq) return SO_ICP_OK;
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  int rc = upload_map(c);
  if (rc) return rc;
  HIP_TRY(c, c->d_q.reserve(nq * 12)); HIP_TRY(c, c->d_nbr.reserve(nq * k * 12)); HIP_TRY(c, c->d_d2.reserve(nq * k * 4));
  HIP_TRY(c, c->d_idx.reserve(nq * k * 4)); HIP_TRY(c, c->d_found.reserve(nq)); HIP_TRY(c, c->d_fblist.reserve(nq * 4));
  HIP_TRY(c, hipMemcpyAsync(c->d_q.p, q, nq * 12, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(c->d_fbcount, 0, 4, c->stream));
  // the 27-cell block certainly covers a ball of one cell edge around the query
  const double cover = (1.0 / c->view.inv_cell) * (1.0 - 1e-5);
  const float gate = (float)(cover * cover);
  launch_knn_only(c->d_q.as<float>(), (uint32_t)nq, k, c->view, gate, c->d_nbr.as<float>(), c->d_d2.as<float>(), c->d_idx.as<int32_t>(),
                  c->d_found.as<uint8_t>(), c->d_fblist.as<uint32_t>(), c->d_fbcount, c->stream);
  HIP_TRY(c, hipMemcpyAsync(c->h_u32, c->d_fbcount, 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const uint32_t n_fb = c->h_u32[0];
  launch_knn_fallback(c->d_q.as<float>(), c->d_fblist.as<uint32_t>(), n_fb, k, c->view, c->d_nbr.as<float>(), c->d_d2.as<float>(), c->d_idx.as<int32_t>(), c->stream);
  HIP_TRY(c, hipMemcpyAsync(nbr, c->d_nbr.p, nq * k * 12, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(d2, c->d_d2.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  if (idx) HIP_TRY(c, hipMemcpyAsync(idx, c->d_idx.p, nq * k * 4, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(found, c->d_found.p, nq, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return SO_ICP_OK;
}

int so_icp_upload_scan(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, void** d_out) {
  if (!c || (!xyz && n) || !d_out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  DevBuf b;
  const int rc = upload_scan_impl(c, xyz, n, stride_bytes, b);
  if (rc) { b.release(); return rc; }
  c->resident_scans.push_back(b);
  *d_out = b.p;
  return SO_ICP_OK;
}

int so_icp_free_scan(so_icp_ctx* c, void* d_scan) {
  if (!c) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  for (size_t i = 0; i < c->resident_scans.size(); ++i)
    if (c->resident_scans[i].p == d_scan) {
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      c->resident_scans[i].release();
      c->resident_scans.erase(c->resident_scans.begin() + i);
      return SO_ICP_OK;
    }
  return fail(c, SO_ICP_E_INVALID, "so_icp_free_scan: unknown scan pointer");
}

int so_icp_register_dev(so_icp_ctx* c, const void* d_scan, size_t n, const double pose_in[7], double pose_out[7], so_icp_stats* st) {
  if (!c) return SO_ICP_E_INVALID;
  if (const int rc = refuse_pending(c, "so_icp_register_dev", kPriorSingle)) return rc;
  const PriorOneShot consume{c};
  if (!pose_in || !pose_out || (!d_scan && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  c->corr_last.valid = false;
  return register_core(c, static_cast<const float*>(d_scan), n, pose_in, pose_out, st);
}

int so_icp_register(so_icp_ctx* c, const float* xyz, size_t n, size_t stride_bytes, const double pose_in[7], double pose_out[7], so_icp_stats* st) {
  if (!c) return SO_ICP_E_INVALID;
  if (const int rc = refuse_pending(c, "so_icp_register", kPriorSingle)) return rc;
  const PriorOneShot consume{c};
  if (!pose_in || !pose_out || (!xyz && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  c->corr_last.valid = false;
  const float* d_scan = nullptr;
  int rc = resolve_scan(c, xyz, n, stride_bytes, &d_scan);  // the copy announced with so_icp_stage_scan, or a plain upload
  if (rc) return rc;
  rc = register_core(c, d_scan, n, pose_in, pose_out, st);
  c->scan_staged = false;
  release_staged(c);
  return rc;
}


// symmetric 3x3 eigen-decomposition (cyclic Jacobi), ascending eigenvalues, eigenvectors in the columns of V
static void eig3_host(const double A[9], double ev[3], double V[9]) {
  double a[9]; std::memcpy(a, A, sizeof(a));
  for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    const double off = a[1] * a[1] + a[2] * a[2] + a[5] * a[5];
    if (off <= 1e-300) break;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        const double apq = a[3 * p + q];
        if (apq == 0.0) continue;
        const double theta = (a[3 * q + q] - a[3 * p + p]) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
        for (int k = 0; k < 3; ++k) {  // A <- A G
          const double akp = a[3 * k + p], akq = a[3 * k + q];
          a[3 * k + p] = cs * akp - sn * akq; a[3 * k + q] = sn * akp + cs * akq;
        }
        for (int k = 0; k < 3; ++k) {  // A <- G^T A
          const double apk = a[3 * p + k], aqk = a[3 * q + k];
          a[3 * p + k] = cs * apk - sn * aqk; a[3 * q + k] = sn * apk + cs * aqk;
        }
        for (int k = 0; k < 3; ++k) {
          const double vkp = V[3 * k + p], vkq = V[3 * k + q];
          V[3 * k + p] = cs * vkp - sn * vkq; V[3 * k + q] = sn * vkp + cs * vkq;
        }
      }
  }
  int idx[3] = {0, 1, 2};
  for (int i = 0; i < 3; ++i) ev[i] = a[4 * i];
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2 - i; ++j)
      if (ev[idx[j]] > ev[idx[j + 1]]) std::swap(idx[j], idx[j + 1]);
  double e2[3], V2[9];
  for (int c2 = 0; c2 < 3; ++c2) { e2[c2] = ev[idx[c2]]; for (int r = 0; r < 3; ++r) V2[3 * r + c2] = V[3 * r + idx[c2]]; }
  std::memcpy(ev, e2, sizeof(e2)); std::memcpy(V, V2, sizeof(V2));
}

int so_icp_registration_error(const so_icp_stats* st, so_icp_registration_error_t* out) {
  if (!st || !out) return SO_ICP_E_INVALID;
  std::memset(out, 0, sizeof(*out));
  // (J^T J)^-1 by Cholesky: L L^T = H, then solve for the six unit vectors
  double L[36];
  for (int j = 0; j < 6; ++j) {
    double d = st->JtJ[6 * j + j];
    for (int k = 0; k < j; ++k) d -= L[6 * j + k] * L[6 * j + k];
    if (!(d > 0.0) || !std::isfinite(d)) return SO_ICP_E_INVALID;
    L[6 * j + j] = std::sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = st->JtJ[6 * i + j];
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      L[6 * i + j] = s / L[6 * j + j];
    }
  }
  for (int c2 = 0; c2 < 6; ++c2) {
    double z[6], x[6];
    for (int i = 0; i < 6; ++i) { double s = (i == c2) ? 1.0 : 0.0; for (int k = 0; k < i; ++k) s -= L[6 * i + k] * z[k]; z[i] = s / L[6 * i + i]; }
    for (int i = 5; i >= 0; --i) { double s = z[i]; for (int k = i + 1; k < 6; ++k) s -= L[6 * k + i] * x[k]; x[i] = s / L[6 * i + i]; }
    for (int r = 0; r < 6; ++r) out->covariance[6 * r + c2] = x[r];
  }
  for (int r = 0; r < 6; ++r)  // symmetrise the rounding
    for (int c2 = r + 1; c2 < 6; ++c2) { const double m = 0.5 * (out->covariance[6 * r + c2] + out->covariance[6 * c2 + r]); out->covariance[6 * r + c2] = out->covariance[6 * c2 + r] = m; }
  double P[9], O[9], ev[3], V[9];
  for (int r = 0; r < 3; ++r) for (int c2 = 0; c2 < 3; ++c2) { P[3 * r + c2] = out->covariance[6 * r + c2]; O[3 * r + c2] = out->covariance[6 * (r + 3) + c2 + 3]; }
  eig3_host(P, ev, V);
  out->position_error = std::sqrt(ev[2]);
  for (int r = 0; r < 3; ++r) out->position_error_direction[r] = V[3 * r + 2];
  out->pos_inverse_condition_num = std::sqrt(ev[0]) / std::sqrt(ev[2]);
  eig3_host(O, ev, V);
  out->orientation_error_deg = std::sqrt(ev[2]) * 180.0 / M_PI;
  for (int r = 0; r < 3; ++r) out->orientation_error_direction[r] = V[3 * r + 2];
  out->ori_inverse_condition_num = std::sqrt(ev[0]) / std::sqrt(ev[2]);
  return SO_ICP_OK;
}


int so_icp_lm_begin(so_icp_lm_state* s, const double x0[7], const so_icp_sums* sums, int max_iterations, double next_pose[7]) {
  if (!s || !x0 || !sums || !next_pose) return SO_ICP_E_INVALID;
  LmState* S = reinterpret_cast<LmState*>(s);
  return lm_begin(*S, x0, *reinterpret_cast<const LmSums*>(sums), max_iterations, next_pose);
}
int so_icp_lm_feed(so_icp_lm_state* s, const so_icp_sums* sums, double next_pose[7]) {
  if (!s || !sums || !next_pose) return SO_ICP_E_INVALID;
  return lm_feed(*reinterpret_cast<LmState*>(s), *reinterpret_cast<const LmSums*>(sums), next_pose);
}
int so_icp_lm_result(const so_icp_lm_state* s, double pose[7], so_icp_iter_stats* st) {
  if (!s || !pose) return SO_ICP_E_INVALID;
  const LmState* S = reinterpret_cast<const LmState*>(s);
  std::memcpy(pose, S->x, 7 * sizeof(double));
  if (st) {
    st->num_surf_from_scan = (int32_t)S->count; st->lm_iterations = S->lm_iterations; st->num_successful_steps = S->num_successful;
    st->termination = S->termination; st->initial_cost = S->initial_cost; st->final_cost = S->x_cost;
  }
  return SO_ICP_OK;
}

int so_icp_get_timing(so_icp_ctx* c, so_icp_timing* t) { if (!c || !t) return SO_ICP_E_INVALID; *t = c->timing; return SO_ICP_OK; }
int so_icp_reset_timing(so_icp_ctx* c) { if (!c) return SO_ICP_E_INVALID; std::memset(&c->timing, 0, sizeof(c->timing)); return SO_ICP_OK; }
int so_icp_set_time_kernels(so_icp_ctx* c, int mode) {
  if (!c || mode < 0 || mode > 2) return SO_ICP_E_INVALID;
  c->cfg.time_kernels = mode;
  return SO_ICP_OK;
}
int so_icp_debug_stamps(so_icp_ctx* c, uint64_t out[16]) {
  if (!c || !out) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  for (int i = 0; i < 16; ++i) out[i] = c->h_state->dbg[i];
  return SO_ICP_OK;
}
int so_icp_debug_knn_stamps(so_icp_ctx* c, uint64_t* out, size_t capacity_words, size_t* n_words) {
  if (!c || !n_words) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  const size_t have = c->d_kdbg.p ? (size_t)2 * kKnnBlocks * 4 * 16 : 0;
  *n_words = have;
  if (!out || !have) return SO_ICP_OK;
  if (capacity_words < have) return fail(c, SO_ICP_E_INVALID, "so_icp_debug_knn_stamps: buffer too small");
  HIP_TRY(c, hipMemcpy(out, c->d_kdbg.p, have * sizeof(uint64_t), hipMemcpyDeviceToHost));
  return SO_ICP_OK;
}
int so_icp_debug_match_status(so_icp_ctx* c, uint8_t* out, size_t n) {
  if (!c || (!out && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (!n) return SO_ICP_OK;
  if (n > c->d_status.cap) return fail(c, SO_ICP_E_INVALID, "so_icp_debug_match_status: more entries than the last scan had");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->d_status.p, n, hipMemcpyDeviceToHost));
  return SO_ICP_OK;
}
int so_icp_debug_neighbours(so_icp_ctx* c, uint32_t* out, size_t n) {
  if (!c || (!out && n)) return SO_ICP_E_INVALID;
  NEED_DEVICE(c);
  if (!n) return SO_ICP_OK;
  if (n * 20 > c->d_nbr5.cap) return fail(c, SO_ICP_E_INVALID, "so_icp_debug_neighbours: more entries than the last scan had");
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(out, c->d_nbr5.p, n * 20, hipMemcpyDeviceToHost));
  return SO_ICP_OK;
}
static_assert(sizeof(so_icp_lm_script_entry) == sizeof(LmScriptEntry) && sizeof(so_icp_lm_script_step) == sizeof(LmScriptStep) &&
              offsetof(so_icp_lm_script_step, hand) == offsetof(LmScriptStep, hand) && offsetof(so_icp_lm_script_step, state) == offsetof(LmScriptStep, S) &&
              SO_ICP_LM_SCRIPT_MAX == kLmScriptMaxEntries && SO_ICP_MAX_OUTER == 16, "so_icp_lm_script_* mirror kernels.h");
int so_icp_debug_lm_script(so_icp_ctx* c, int form, const double x0[7], int lm_max, int max_outer, int outer_iter, const so_icp_lm_script_entry* entries,
                           int n_entries, uint64_t want, so_icp_lm_script_step* steps, so_icp_lm_script_result* result) {
  if (!c) return SO_ICP_E_INVALID;
  if (!x0 || !entries || !steps || !result || (form != 0 && form != 1) || n_entries < 1 || n_entries > SO_ICP_LM_SCRIPT_MAX || lm_max < 0 ||
      max_outer < 1 || outer_iter < 0)
    return fail(c, SO_ICP_E_INVALID, "so_icp_debug_lm_script: bad argument");
  NEED_DEVICE(c);
  HIP_TRY(c, hipSetDevice(c->cfg.device_id));
  struct Scratch {  // owned by this call, whatever way it returns
    DevBuf state, entries, steps, hist;
    ~Scratch() { state.release(); entries.release(); steps.release(); hist.release(); }
  } sc;
  const size_t hist_bytes = (size_t)kHistReplicas * kHistStride * sizeof(int32_t);
  HIP_TRY(c, sc.state.reserve(sizeof(DevState)));
  HIP_TRY(c, sc.entries.reserve((size_t)n_entries * sizeof(LmScriptEntry)));
  HIP_TRY(c, sc.steps.reserve((size_t)n_entries * sizeof(LmScriptStep)));
  HIP_TRY(c, sc.hist.reserve(hist_bytes));
  std::vector<unsigned char> init(sizeof(DevState), 0);
  DevState* h = reinterpret_cast<DevState*>(init.data());
  for (int i = 0; i < 7; ++i) { h->pose_in[i] = x0[i]; h->T[i] = x0[i]; h->eval_pose[i] = x0[i]; }
  h->max_outer = max_outer; h->lm_max = lm_max; h->outer_iter = outer_iter; h->n_iterations = outer_iter;
  hipStream_t s = c->stream;
  DevState* ds = sc.state.as<DevState>();
  LmScriptEntry* de = sc.entries.as<LmScriptEntry>();
  LmScriptStep* dstep = sc.steps.as<LmScriptStep>();
  HIP_TRY(c, hipMemcpyAsync(ds, h, sizeof(DevState), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(de, entries, (size_t)n_entries * sizeof(LmScriptEntry), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemsetAsync(dstep, 0xFF, (size_t)n_entries * sizeof(LmScriptStep), s));
  HIP_TRY(c, hipMemsetAsync(sc.hist.p, 0, hist_bytes, s));
  if (form == 0) {
    launch_lm_script_wave(ds, de, n_entries, (unsigned long long)want, dstep, s);
  } else {
    const EvalParams ep = eval_params(0.2f, 0, 0);  // (hring == nullptr: the step kernel publishes nothing)
    int slot = 0;
    for (int e = 0; e < n_entries; ++e) {
      slot = entries[e].new_solve ? 0 : slot + 1;
      launch_lm_step(slot, ds, &de[e].sums, sc.hist.as<int32_t>(), ep, s);
      launch_lm_script_record(ds, dstep + e, s);
    }
  }
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(steps, dstep, (size_t)n_entries * sizeof(LmScriptStep), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(h, ds, sizeof(DevState), hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  std::memset(result, 0, sizeof(*result));
  std::memcpy(&result->state, &h->S, sizeof(LmState));
  std::memcpy(result->T, h->T, sizeof(h->T)); std::memcpy(result->eval_pose, h->eval_pose, sizeof(h->eval_pose));
  std::memcpy(result->T_final, h->T_final, sizeof(h->T_final));
  std::memcpy(result->JtJ, h->JtJ, sizeof(h->JtJ)); std::memcpy(result->Jtr, h->Jtr, sizeof(h->Jtr));
  result->lm_more = h->lm_more; result->outer_iter = h->outer_iter; result->n_iterations = h->n_iterations; result->reg_done = h->reg_done;
  result->done_count = h->done_count;
  for (int o = 0; o < 16; ++o) {
    const DevIterStats& d = h->iters[o];
    so_icp_iter_stats& t = result->iterations[o];
    t.translation_norm = d.translation_norm; t.rotation_norm = d.rotation_norm; t.num_surf_from_scan = d.num_surf;
    t.lm_iterations = d.lm_iterations; t.num_successful_steps = d.num_successful; t.termination = d.termination;
    t.initial_cost = d.initial_cost; t.final_cost = d.final_cost;
    std::memcpy(t.reject_hist, d.reject_hist, sizeof(d.reject_hist)); std::memcpy(t.obs_hist, d.obs_hist, sizeof(d.obs_hist));
    std::memcpy(t.pose_after, d.pose_after, sizeof(d.pose_after));
  }
  return SO_ICP_OK;
}
int so_icp_synchronize(so_icp_ctx* c) { if (!c) return SO_ICP_E_INVALID; NEED_DEVICE(c); HIP_TRY(c, hipStreamSynchronize(c->stream)); return SO_ICP_OK; }

}  // extern "C"
