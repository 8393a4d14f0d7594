// feature_kernels.hip -- featureExtraction's per-sweep point work (src/FeatureExtraction/featureExtraction.cpp) on the device:
//   ingest_deskew_kernel  laserCloudHandler's pcl::fromROSMsg (+ utils::transformOusterPoints and the ns -> s time for the Ouster,
//                         :710-766, superodom_utils.cpp:202-209) fused with removePointDistortion (:223-314): payload in,
//                         point_os::PointcloudXYZITR records out (the LaserFeature's cloud_nodistortion)
//   surf_sample_kernel    uniformFeatureExtraction (:504-525): an order-preserving compaction into pcl::PointXYZI records
//                         (cloud_surface), one launch with a decoupled look-back across workgroups
// and, for the records that pass leaves in HBM, laserMapping::publishTopic's registered scan (src/LaserMapping/laserMapping.cpp:464-493):
//   registered_scan_kernel  utils::pointAssociateToMap over the cloud and the drop of points at the world origin, compacted
// The de-skew arithmetic is deskew_math.h's, as in map_kernels.hip deskew_kernel: the same header functions in the same order,
// so the records equal that kernel's run on the ingested sweep bit for bit.
#include <hip/hip_runtime.h>

#include <initializer_list>
#include <type_traits>

#include "deskew_math.h"
#include "device_idioms.h"
#include "feature_kernels.h"
#include "so_math.h"
#include "untimed_math.h"

namespace soicp {

// PointCloud2 fields sit at any byte offset (velodyne_pointcloud's time is at 18 of a 22-byte point); A4: every offset, step
// and the base are multiples of 4, so the fields load as dwords
template <bool A4, typename T>
__device__ __forceinline__ T load_field(const uint8_t* p) {
  if (A4) return *reinterpret_cast<const T*>(p);
  T v;
  __builtin_memcpy(&v, p, sizeof(T));
  return v;
}

// A4 of the three ingests: the base, the steps and every present offset (< 0: absent) are multiples of 4
static bool dword_aligned(const void* base, std::initializer_list<uint32_t> steps, std::initializer_list<int32_t> offsets) {
  bool a4 = reinterpret_cast<uintptr_t>(base) % 4u == 0;
  for (uint32_t step : steps) a4 = a4 && step % 4u == 0;
  for (int32_t off : offsets) a4 = a4 && (off < 0 || off % 4 == 0);
  return a4;
}

// The instantiation of an ingest kernel: launch(A4, DESKEW, LDS) with the three as compile-time constants (std::bool_constant).
// No pose, no de-skew; up to kDeskewLdsPoses poses, the table in LDS; more, the table read from global memory.
template <typename Launch>
static void dispatch_ingest(bool a4, uint32_t n_poses, Launch&& launch) {
  auto with_a4 = [&](auto A4) {
    if (!n_poses) launch(A4, std::false_type{}, std::false_type{});
    else if (n_poses <= kDeskewLdsPoses) launch(A4, std::true_type{}, std::true_type{});
    else launch(A4, std::true_type{}, std::false_type{});
  };
  if (a4) with_a4(std::true_type{});
  else with_a4(std::false_type{});
}

template <bool A4, bool DESKEW, bool LDS>
__global__ __launch_bounds__(256) void ingest_deskew_kernel(const uint8_t* __restrict__ raw, uint32_t n, SweepFields sf, uint8_t* __restrict__ out,
                                                            double t0, const double* __restrict__ poses, uint32_t n_poses, DeskewFrames f,
                                                            uint32_t* __restrict__ n_clamped) {
  __shared__ double tab_lds[(DESKEW && LDS) ? kDeskewLdsPoses * kStampedPoseDoubles : 1];
  if (DESKEW && LDS) {
    copy_pose_table(tab_lds, poses, n_poses);
    __syncthreads();
  }
  const double* tab = (DESKEW && LDS) ? tab_lds : poses;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool clamped = false;
  if (i < n) {
    const uint32_t row = i / sf.width, col = i - row * sf.width;  // row-major, rows row_step apart (pcl::fromROSMsg)
    const uint8_t* p = raw + (size_t)row * sf.row_step + (size_t)col * sf.point_step;
    // a field PCL does not match keeps the value-initialised point's 0
    float x = sf.x >= 0 ? load_field<A4, float>(p + sf.x) : 0.0f;
    float y = sf.y >= 0 ? load_field<A4, float>(p + sf.y) : 0.0f;
    float z = sf.z >= 0 ? load_field<A4, float>(p + sf.z) : 0.0f;
    const float intensity = sf.intensity >= 0 ? load_field<A4, float>(p + sf.intensity) : 0.0f;
    float time;
    uint32_t ring;
    if (sf.ouster) {
      // transformOusterPoints: Vector3d(x, y, z), rot * p + pos in fp64 (Eigen's _transformVector), rounded to float
      double ox, oy, oz;
      quat_rotate<double>(sf.ouster_q, (double)x, (double)y, (double)z, ox, oy, oz);
      x = (float)(ox + sf.ouster_t[0]); y = (float)(oy + sf.ouster_t[1]); z = (float)(oz + sf.ouster_t[2]);
      const uint32_t t = sf.time >= 0 ? load_field<A4, uint32_t>(p + sf.time) : 0u;
      time = (float)t * 1e-9f;  // dst.time = src.t * 1e-9f
      ring = 0u;
    } else {
      time = sf.time >= 0 ? load_field<A4, float>(p + sf.time) : 0.0f;
      ring = sf.ring >= 0 ? (uint32_t)load_field<A4, uint16_t>(p + sf.ring) : 0u;
    }
    if (DESKEW) clamped = deskew_point(tab, n_poses, t0, time, f, x, y, z);  // removePointDistortion, :293-306 (as deskew_kernel)
    // PointcloudXYZITR: x y z, data[3] = 0, intensity, time, ring (uint16) and zero padding
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * kFeatureRecordBytes);
    o[0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
    o[1] = make_uint4(__float_as_uint(intensity), __float_as_uint(time), ring, 0u);
  }
  if (DESKEW) wave_count_add(clamped, n_clamped);
}

void launch_ingest_deskew(const uint8_t* d_raw, uint32_t n, const SweepFields& sf, uint8_t* d_rec, double t0, const double* d_poses,
                          uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, hipStream_t s) {
  if (!n) return;
  const bool a4 = dword_aligned(d_raw, {sf.point_step, sf.row_step}, {sf.x, sf.y, sf.z, sf.intensity, sf.time, sf.ring});
  dispatch_ingest(a4, n_poses, [&](auto A4, auto DESKEW, auto LDS) {
    ingest_deskew_kernel<A4(), DESKEW(), LDS()><<<(n + 255u) / 256u, 256, 0, s>>>(d_raw, n, sf, d_rec, t0, d_poses, n_poses, f, d_n_clamped);
  });
}

// livoxHandler's loop (:794-806) fused with removePointDistortion, a kernel of its own beside ingest_deskew_kernel (whose code
// it leaves as it is): one thread per livox_ros_driver2 CustomPoint, the same records out.  A4: base, point_step and the offsets
// of the four 4-byte fields are multiples of 4, those load as dwords; the three uint8 fields are byte loads either way, so nothing
// behind a point's last field is read (the last CustomPoint of a CDR sequence has 19 bytes, not 20).
template <bool A4, bool DESKEW, bool LDS>
__global__ __launch_bounds__(256) void livox_ingest_deskew_kernel(const uint8_t* __restrict__ raw, uint32_t n, LivoxFields lf, uint8_t* __restrict__ out,
                                                                  double t0, const double* __restrict__ poses, uint32_t n_poses, DeskewFrames f,
                                                                  uint32_t* __restrict__ n_clamped) {
  __shared__ double tab_lds[(DESKEW && LDS) ? kDeskewLdsPoses * kStampedPoseDoubles : 1];
  if (DESKEW && LDS) {
    copy_pose_table(tab_lds, poses, n_poses);
    __syncthreads();
  }
  const double* tab = (DESKEW && LDS) ? tab_lds : poses;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool clamped = false;
  if (i < n) {
    const uint8_t* p = raw + (size_t)i * lf.point_step;
    const uint32_t line = p[lf.line], tag = p[lf.tag] & 0x30u;
    // a point the handler skips keeps the value-initialised record of points.resize(point_num)
    float x = 0.0f, y = 0.0f, z = 0.0f, intensity = 0.0f, time = 0.0f;
    uint32_t ring = 0u;
    if (line < lf.n_scans && (tag == 0x10u || tag == 0x00u)) {
      // rotation_matrix * Vector3d(x, y, z): Eigen's coefficient product, left to right, unfused (-ffp-contract=off); rounded to float
      const double px = (double)load_field<A4, float>(p + lf.x), py = (double)load_field<A4, float>(p + lf.y),
                   pz = (double)load_field<A4, float>(p + lf.z);
      x = (float)((lf.R[0] * px + lf.R[1] * py) + lf.R[2] * pz);
      y = (float)((lf.R[3] * px + lf.R[4] * py) + lf.R[5] * pz);
      z = (float)((lf.R[6] * px + lf.R[7] * py) + lf.R[8] * pz);
      intensity = (float)p[lf.reflectivity];
      time = __fdiv_rn((float)load_field<A4, uint32_t>(p + lf.offset_time), 1000000000.0f);  // offset_time / float(1000000000), :803
      ring = line;
    }
    if (DESKEW) clamped = deskew_point(tab, n_poses, t0, time, f, x, y, z);  // removePointDistortion, :293-306: the zero records too
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)i * kFeatureRecordBytes);
    o[0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
    o[1] = make_uint4(__float_as_uint(intensity), __float_as_uint(time), ring, 0u);
  }
  if (DESKEW) wave_count_add(clamped, n_clamped);
}

void launch_livox_ingest_deskew(const uint8_t* d_raw, uint32_t n, const LivoxFields& lf, uint8_t* d_rec, double t0, const double* d_poses,
                                uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, hipStream_t s) {
  if (!n) return;
  const bool a4 = dword_aligned(d_raw, {lf.point_step}, {(int32_t)lf.offset_time, (int32_t)lf.x, (int32_t)lf.y, (int32_t)lf.z});
  dispatch_ingest(a4, n_poses, [&](auto A4, auto DESKEW, auto LDS) {
    livox_ingest_deskew_kernel<A4(), DESKEW(), LDS()><<<(n + 255u) / 256u, 256, 0, s>>>(d_raw, n, lf, d_rec, t0, d_poses, n_poses, f, d_n_clamped);
  });
}

// uniformFeatureExtraction, featureExtraction.cpp:507-522: candidates i = 1, 1 + s, 1 + 2s, ... < n, each against the RAW record
// i - 1, kept when  |dx| > 1e-7 || |dy| > 1e-7 || (|dz| > 1e-7 && x*x + y*y + z*z > r*r)  -- C++ precedence: the range gate only
// goes with the z test.  The differences and abs are float (the float overload), compared in double; the squared norm and r*r are
// float, left to right, unfused (-ffp-contract=off).  A NaN neighbour makes every term false.
__device__ __forceinline__ bool surf_keep(const float4 a, const float4 b, float min_range) {
  const float dx = fabsf(a.x - b.x), dy = fabsf(a.y - b.y), dz = fabsf(a.z - b.z);
  const float r2 = min_range * min_range;
  return ((double)dx > 1e-7) || ((double)dy > 1e-7) || (((double)dz > 1e-7) && (a.x * a.x + a.y * a.y + a.z * a.z > r2));
}

// One launch: each workgroup takes kSurfItems candidates in ticket order (kPer rounds of 256 consecutive candidates: the loads of a
// wavefront are 64 neighbouring records), ranks its kept ones with a ballot + mbcnt per round and an LDS prefix over (round,
// wavefront), and finds the number kept in front of it with a decoupled look-back (records = flag << 62 | value, all zero
// before the launch, vector atomics at agent scope; see leaf_heads_scan_kernel).  Output pcl::PointXYZI in ascending i: x y z,
// data[3] = 1 (PCL's constructor), intensity = the record's time, zero padding.  The last workgroup writes the count.
__global__ __launch_bounds__(256) void surf_sample_kernel(const uint8_t* __restrict__ rec, uint32_t n_cand, uint32_t step, float min_range,
                                                          uint8_t* __restrict__ surf, uint32_t* __restrict__ n_surf,
                                                          unsigned long long* __restrict__ state, uint32_t* __restrict__ ticket, uint32_t nblk) {
  constexpr int kPer = (int)(kSurfItems / 256u);
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  const float4* r4 = reinterpret_cast<const float4*>(rec);
  unsigned long long bal[kPer];
  float4 pt[kPer];
  float tm[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t k = bid * kSurfItems + (uint32_t)q * 256u + (uint32_t)tid;
    bool keep = false;
    pt[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); tm[q] = 0.0f;
    if (k < n_cand) {
      const size_t i = 1u + (size_t)k * step;
      pt[q] = r4[2 * i];
      tm[q] = r4[2 * i + 1].y;
      keep = surf_keep(pt[q], r4[2 * (i - 1)], min_range);
    }
    bal[q] = __ballot(keep);
    if (lane == 0) s_pre[q * 4 + wave] = (uint32_t)__popcll(bal[q]);
  }
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in candidate order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    if (lane == 0) __hip_atomic_store(&state[bid], ((bid == 0u ? 2ull : 1ull) << 62) | (unsigned long long)agg, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t excl = 0;
    int base = (int)bid - 1;
    while (base >= 0) {
      const int j = base - lane;
      unsigned long long r = 2ull << 62;
      if (j >= 0) {
        do { r = __hip_atomic_load(&state[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((r >> 62) == 0ull);
      }
      const unsigned long long mi = __ballot((r >> 62) == 2ull);
      const int first = mi ? __ffsll((long long)mi) - 1 : 64;
      uint32_t contrib = lane <= first ? (uint32_t)(r & 0xFFFFFFFFull) : 0u;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) contrib += (uint32_t)__shfl_xor((int)contrib, d, 64);
      excl += contrib;
      if (mi) break;
      base -= 64;
    }
    if (lane == 0) {
      if (bid != 0u) __hip_atomic_store(&state[bid], (2ull << 62) | (unsigned long long)(excl + agg), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (bid == nblk - 1u) *n_surf = excl + agg;
      s_excl = excl;
    }
  }
  __syncthreads();
  const uint32_t excl = s_excl;
  uint4* o4 = reinterpret_cast<uint4*>(surf);
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    if ((bal[q] >> lane) & 1ull) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[q], 0u));
      const size_t at = (size_t)excl + s_pre[q * 4 + wave] + below;
      o4[2 * at] = make_uint4(__float_as_uint(pt[q].x), __float_as_uint(pt[q].y), __float_as_uint(pt[q].z), __float_as_uint(1.0f));
      o4[2 * at + 1] = make_uint4(__float_as_uint(tm[q]), 0u, 0u, 0u);
    }
  }
}

void launch_surf_sample(const uint8_t* d_rec, uint32_t n, uint32_t step, float min_range, uint8_t* d_surf, uint32_t* d_n_surf,
                        unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s) {
  const uint32_t nblk = surf_workgroups(n, step);
  if (!nblk) return;
  surf_sample_kernel<<<nblk, 256, 0, s>>>(d_rec, surf_candidates(n, step), step, min_range, d_surf, d_n_surf, d_state, d_ticket, nblk);
}

// laserMapping::publishTopic's registered scan (laserMapping.cpp:464-493, utils::pointAssociateToMap, superodom_utils.cpp:148-158)
// from records that stay as they are: transform_cloud_kernel's arithmetic (map_kernels.hip) -- a point within 0.1 m of the sensor
// keeps its coordinates, every other one becomes q * p + t in fp64, rounded to float; kept when the result lies farther than
// 0.1 m from the world origin; float products and sums, compared with the double 0.01 -- and surf_sample_kernel's order-preserving
// compaction: tiles of kSurfItems consecutive records in ticket order, a ballot + mbcnt per round, the LDS prefix over (round,
// wavefront), lookback_exclusive, the count from the last workgroup.  A kept record goes out as all its `stride` bytes with the
// three floats replaced.  V16: rec and out 16-byte aligned and stride a multiple of 16 -- 16-byte loads and stores, the first two
// of a record held in registers from the first pass (all of a 32-byte record); otherwise dwords (stride a multiple of 4).
template <bool V16>
__global__ __launch_bounds__(256) void registered_scan_kernel(const uint8_t* __restrict__ rec, uint32_t n, uint32_t stride, Pose pose,
                                                              uint8_t* __restrict__ out, uint32_t* __restrict__ n_kept,
                                                              unsigned long long* __restrict__ state, uint32_t* __restrict__ ticket, uint32_t nblk) {
  constexpr int kPer = (int)(kSurfItems / 256u);
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(ticket, 1u);
  __syncthreads();
  const uint32_t bid = s_bid;
  unsigned long long bal[kPer];
  uint4 head[kPer];                // x' y' z' and, V16, the record's fourth word
  uint4 tail[V16 ? kPer : 1];      // V16, stride >= 32: bytes 16 .. 31
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kSurfItems + (uint32_t)q * 256u + (uint32_t)tid;
    bool keep = false;
    head[q] = make_uint4(0u, 0u, 0u, 0u);
    if (V16) tail[q] = make_uint4(0u, 0u, 0u, 0u);
    if (i < n) {
      const uint8_t* p = rec + (size_t)i * stride;
      if (V16) {
        head[q] = *reinterpret_cast<const uint4*>(p);
        if (stride >= 32u) tail[q] = *reinterpret_cast<const uint4*>(p + 16);
      } else {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
        head[q].x = w[0]; head[q].y = w[1]; head[q].z = w[2];
      }
      float x = __uint_as_float(head[q].x), y = __uint_as_float(head[q].y), z = __uint_as_float(head[q].z);
      if (!(x * x + y * y + z * z < 0.01)) {
        double wx, wy, wz;
        quat_rotate<double>(pose.q, (double)x, (double)y, (double)z, wx, wy, wz);
        x = (float)(wx + pose.t[0]); y = (float)(wy + pose.t[1]); z = (float)(wz + pose.t[2]);
        head[q].x = __float_as_uint(x); head[q].y = __float_as_uint(y); head[q].z = __float_as_uint(z);
      }
      keep = x * x + y * y + z * z > 0.01;
    }
    bal[q] = __ballot(keep);
    if (lane == 0) s_pre[q * 4 + wave] = (uint32_t)__popcll(bal[q]);
  }
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in record order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    const uint32_t excl = lookback_exclusive(state, bid, agg, lane);
    if (lane == 0) {
      if (bid == nblk - 1u) *n_kept = excl + agg;
      s_excl = excl;
    }
  }
  __syncthreads();
  const uint32_t excl = s_excl;
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    if ((bal[q] >> lane) & 1ull) {
      const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal[q] >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal[q], 0u));
      const size_t at = (size_t)excl + s_pre[q * 4 + wave] + below;
      const uint8_t* p = rec + (size_t)(bid * kSurfItems + (uint32_t)q * 256u + (uint32_t)tid) * stride;
      uint8_t* o = out + at * stride;
      if (V16) {
        *reinterpret_cast<uint4*>(o) = head[q];
        if (stride >= 32u) *reinterpret_cast<uint4*>(o + 16) = tail[q];
        for (uint32_t b = 32u; b < stride; b += 16u) *reinterpret_cast<uint4*>(o + b) = *reinterpret_cast<const uint4*>(p + b);
      } else {
        uint32_t* ow = reinterpret_cast<uint32_t*>(o);
        ow[0] = head[q].x; ow[1] = head[q].y; ow[2] = head[q].z;
        for (uint32_t b = 12u; b < stride; b += 4u) *reinterpret_cast<uint32_t*>(o + b) = *reinterpret_cast<const uint32_t*>(p + b);
      }
    }
  }
}

void launch_registered_scan(const uint8_t* d_rec, uint32_t n, uint32_t stride, const Pose& pose, uint8_t* d_out, uint32_t* d_n_kept,
                            unsigned long long* d_state, uint32_t* d_ticket, hipStream_t s) {
  const uint32_t nblk = registered_scan_workgroups(n);
  if (!nblk) return;
  const bool v16 = stride % 16u == 0 && (reinterpret_cast<uintptr_t>(d_rec) | reinterpret_cast<uintptr_t>(d_out)) % 16u == 0;
  if (v16) registered_scan_kernel<true><<<nblk, 256, 0, s>>>(d_rec, n, stride, pose, d_out, d_n_kept, d_state, d_ticket, nblk);
  else registered_scan_kernel<false><<<nblk, 256, 0, s>>>(d_rec, n, stride, pose, d_out, d_n_kept, d_state, d_ticket, nblk);
}

// assignTimeforPointCloud (:646-708) -- the ingest of a sweep whose points carry x y z intensity only (provide_point_time: 0) --
// fused with removePointDistortion, a kernel of its own beside the two ingests above (whose code it leaves as it is).  The ring,
// the drop test and the time are untimed_math.h's.  The reference's loop shrinks its own bound with every drop (cloud_size--), so
// with D(i) = the number of dropped points among [0, i): index i is visited iff i + D(i) < n (i + D(i) increases strictly, so the
// visited indices are a prefix), a visited point that is not dropped is record i - D(i), and the number of records is
// F - D(F) for the first unvisited F -- written by the thread of F - 1, the one visited index whose successor is not.
// registered_scan_kernel's order-preserving compaction over the DROPPED points gives D(i): tiles of kSurfItems consecutive
// points in ticket order, a ballot per round, the LDS prefix over (round, wavefront), lookback_exclusive, mbcnt.  Pass 1 reads
// x y z and keeps one byte per round (the ring, 0xFF = dropped); pass 2, behind the look-back, reads the point again, and only a
// point that becomes a record is de-skewed (deskew_math.h's deskew_point, as the other ingests) and counted in n_clamped: the
// de-skew chain is in the code once, not once per round, and the eight rounds hold 2 registers instead of 48.
template <bool A4, bool DESKEW, bool LDS>
__global__ __launch_bounds__(256) void untimed_ingest_deskew_kernel(const uint8_t* __restrict__ raw, uint32_t n, UntimedFields uf, uint8_t* __restrict__ out,
                                                                    double t0, const double* __restrict__ poses, uint32_t n_poses, DeskewFrames f,
                                                                    uint32_t* __restrict__ n_clamped, uint32_t* __restrict__ n_kept,
                                                                    unsigned long long* __restrict__ state, uint32_t* __restrict__ ticket) {
  constexpr int kPer = (int)(kSurfItems / 256u);
  static_assert(kPer <= 8, "rings holds one byte per round in a 64-bit word");
  __shared__ double tab_lds[(DESKEW && LDS) ? kDeskewLdsPoses * kStampedPoseDoubles : 1];
  __shared__ uint32_t s_bid, s_pre[kPer * 4], s_agg, s_excl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) s_bid = atomicAdd(ticket, 1u);
  if (DESKEW && LDS) copy_pose_table(tab_lds, poses, n_poses);
  __syncthreads();
  const double* tab = (DESKEW && LDS) ? tab_lds : poses;
  const uint32_t bid = s_bid;
  const bool tabled = uf.n_scans == 16u || uf.n_scans == 32u || uf.n_scans == 64u;  // any other value: ring 0, nothing dropped
  unsigned long long rings = 0ull;  // byte q: the ring of this thread's point of round q, 0xFF when it is dropped
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kSurfItems + (uint32_t)q * 256u + (uint32_t)tid;
    int id = 0;
    if (tabled && i < n) {
      const uint32_t row = i / uf.width, col = i - row * uf.width;  // row-major, rows row_step apart (pcl::fromROSMsg)
      const uint8_t* p = raw + (size_t)row * uf.row_step + (size_t)col * uf.point_step;
      const float x = uf.x >= 0 ? load_field<A4, float>(p + uf.x) : 0.0f;
      const float y = uf.y >= 0 ? load_field<A4, float>(p + uf.y) : 0.0f;
      const float z = uf.z >= 0 ? load_field<A4, float>(p + uf.z) : 0.0f;
      id = untimed_ring(untimed_angle(x, y, z), (int)uf.n_scans);
    }
    rings |= (unsigned long long)((uint32_t)id & 0xFFu) << (8 * q);
    const unsigned long long dropped = __ballot(id == kUntimedDropped);
    if (lane == 0) s_pre[q * 4 + wave] = (uint32_t)__popcll(dropped);
  }
  __syncthreads();
  if (tid == 0) {  // exclusive prefix in point order: round-major, then wavefront
    uint32_t acc = 0;
    for (int k = 0; k < kPer * 4; ++k) { const uint32_t v = s_pre[k]; s_pre[k] = acc; acc += v; }
    s_agg = acc;
  }
  __syncthreads();
  const uint32_t agg = s_agg;
  if (wave == 0) {
    const uint32_t excl = lookback_exclusive(state, bid, agg, lane);
    if (lane == 0) s_excl = excl;
  }
  __syncthreads();
  const uint32_t excl = s_excl;
  uint32_t wave_clamped = 0;
  constexpr int kUnroll = DESKEW ? 1 : kPer;  // the de-skew chain once in the code
#pragma unroll kUnroll
  for (int q = 0; q < kPer; ++q) {
    const uint32_t i = bid * kSurfItems + (uint32_t)q * 256u + (uint32_t)tid;
    const uint32_t ring = (uint32_t)(rings >> (8 * q)) & 0xFFu;
    const bool drop = ring == 0xFFu;
    const unsigned long long dropped = __ballot(drop);
    const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(dropped >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)dropped, 0u));
    const uint32_t d = excl + s_pre[q * 4 + wave] + below;  // D(i)
    bool clamped = false;
    if (i < n && i + d < n) {  // visited
      if (!drop) {
        const uint32_t row = i / uf.width, col = i - row * uf.width;
        const uint8_t* p = raw + (size_t)row * uf.row_step + (size_t)col * uf.point_step;
        // a field PCL does not match keeps the value-initialised point's 0
        float x = uf.x >= 0 ? load_field<A4, float>(p + uf.x) : 0.0f;
        float y = uf.y >= 0 ? load_field<A4, float>(p + uf.y) : 0.0f;
        float z = uf.z >= 0 ? load_field<A4, float>(p + uf.z) : 0.0f;
        const float intensity = uf.intensity >= 0 ? load_field<A4, float>(p + uf.intensity) : 0.0f;
        const float time = untimed_time(i, uf.n_scans);
        if (DESKEW) clamped = deskew_point(tab, n_poses, t0, time, f, x, y, z);  // removePointDistortion, :293-306
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)(i - d) * kFeatureRecordBytes);
        o[0] = make_uint4(__float_as_uint(x), __float_as_uint(y), __float_as_uint(z), 0u);
        o[1] = make_uint4(__float_as_uint(intensity), __float_as_uint(time), ring, 0u);
      }
      const uint32_t d_next = d + (drop ? 1u : 0u);  // D(i + 1)
      if (i + 1u + d_next >= n) *n_kept = i + 1u - d_next;  // i + 1 is the first unvisited index
    }
    if (DESKEW) {
      const unsigned long long m = __ballot(clamped);
      wave_clamped += (uint32_t)__popcll(m);
    }
  }
  if (DESKEW && lane == 0 && wave_clamped) atomicAdd(n_clamped, wave_clamped);
}

void launch_untimed_ingest_deskew(const uint8_t* d_raw, uint32_t n, const UntimedFields& uf, uint8_t* d_rec, double t0, const double* d_poses,
                                  uint32_t n_poses, const DeskewFrames& f, uint32_t* d_n_clamped, uint32_t* d_n_kept, unsigned long long* d_state,
                                  uint32_t* d_ticket, hipStream_t s) {
  if (!n) return;
  const bool a4 = dword_aligned(d_raw, {uf.point_step, uf.row_step}, {uf.x, uf.y, uf.z, uf.intensity});
  dispatch_ingest(a4, n_poses, [&](auto A4, auto DESKEW, auto LDS) {
    untimed_ingest_deskew_kernel<A4(), DESKEW(), LDS()><<<untimed_workgroups(n), 256, 0, s>>>(d_raw, n, uf, d_rec, t0, d_poses, n_poses, f, d_n_clamped,
                                                                                            d_n_kept, d_state, d_ticket);
  });
}

}  // namespace soicp
