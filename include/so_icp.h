/*
 * so_icp.h -- C ABI of libsoicp: the MI355X-native (gfx950 / HIP) scan-to-map ICP hot path that
 * replaces, behind the reference's own member-function seams, the CPU path
 *
 *     LidarSLAM::Localization -> performLocalizationAndMapping      (Seam A)
 *     LocalMap::nearestKSearchSurf                                  (Seam B)
 *
 * of superxslam/SuperOdom.  The reference has no plugin/FFI interface, so every
 * entry point below names the reference member function it stands in for.  Citations are relative
 * to /root/reference/super_odometry/ with the short names
 *     LS.cpp = src/LidarProcess/LidarSlam.cpp          LS.h = include/super_odometry/LidarProcess/LidarSlam.h
 *     LM.h   = include/super_odometry/LidarProcess/LocalMap.h
 *     lmap.cpp = src/LaserMapping/laserMapping.cpp
 *
 * Conventions: plain pointers and sizes, no C++/torch types; `int` status (0 ok, >0 soft
 * condition, <0 error; text via so_icp_last_error); nothing throws across the boundary; the caller
 * owns every buffer; a context is single-caller (the reference's LidarSLAM is non-re-entrant,
 * LS.cpp:7-9) and owns its HIP stream, device buffers and (optionally) its RCCL communicator.
 * Pose layout = the reference's pose_parameters[7] (LS.cpp:7-9): {tx,ty,tz, qx,qy,qz,qw}.
 * INTEGRATION.md shows the LidarSLAM-side adapter a maintainer would add.
 */
#ifndef SO_ICP_H
#define SO_ICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SO_ICP_ABI_VERSION 4 /* v4: so_icp_register_sequence; so_icp_timing grew (seq_chained, seq_chain_breaks).  v3: the config, timing and prefilter-info structs grew (shard_mode, solve_workgroups, staging / packing counters, statistic_in_input_order) */

/* LocalMap geometry, LM.h:131-138 */
#define SO_ICP_MAP_W 21
#define SO_ICP_MAP_H 21
#define SO_ICP_MAP_D 11
#define SO_ICP_MAP_NUM 4851
#define SO_ICP_MAX_OUTER 16

/* status codes */
#define SO_ICP_OK 0
#define SO_ICP_NOT_ENOUGH_MAP_FEATURES 1 /* LS.cpp:113-116: surf_from_map_num <= 50, pose = guess */
#define SO_ICP_MAP_SEEDED 2              /* Localization(initialization=false): LS.cpp:45-46, 83-94 */
#define SO_ICP_STAGE_DECLINED 3          /* so_icp_stage_scan: every staging slot holds a scan that is still needed; not staged (soft) */
#define SO_ICP_E_INVALID (-1)
#define SO_ICP_E_HIP (-2)
#define SO_ICP_E_NOMEM (-3)
#define SO_ICP_E_RCCL (-4)
#define SO_ICP_E_UNSUPPORTED (-5)

/* MatchingResult, LS.h:85-94 (index into so_icp_iter_stats.reject_hist) */
enum {
  SO_ICP_MATCH_SUCCESS = 0,
  SO_ICP_MATCH_NOT_ENOUGH_NEIGHBORS = 1,
  SO_ICP_MATCH_NEIGHBORS_TOO_FAR = 2,
  SO_ICP_MATCH_BAD_PCA_STRUCTURE = 3,
  SO_ICP_MATCH_INVALID_NUMERICAL = 4,
  SO_ICP_MATCH_MSE_TOO_LARGE = 5,
  SO_ICP_MATCH_UNKNOWN = 6,
  SO_ICP_N_REJECT = 7
};
#define SO_ICP_N_OBS 9 /* Feature_observability, LS.h:96-107 */

typedef struct so_icp_ctx so_icp_ctx;

/* Knobs the node pushes into LidarSLAM before each call (lmap.cpp:103-120, 648-649, 703-711) plus
 * device placement.  Fill with so_icp_default_config() first. */
typedef struct {
  int32_t abi_version;          /* SO_ICP_ABI_VERSION */
  int32_t device_id;            /* HIP device ordinal (one process per GPU); < 0: host-only context -- LocalMap
                                   bookkeeping works, every compute entry point returns SO_ICP_E_HIP (no CPU fallback) */
  int32_t rank, world_size;     /* map shard owned by this context (brick-hash of the voxel grid) */
  int32_t max_iterations;       /* LocalizationICPMaxIter (LS.h:273; YAML max_iterations: 5) */
  int32_t lm_max_iterations;    /* ceres max_num_iterations = 4 (LS.cpp:232) */
  int32_t max_surface_features; /* OptSet.max_surface_features (LS.cpp:346-359); < 0: use all points (the reference compares
                                   size_t > int: a negative value never samples); 0 drops every point, like the reference */
  int32_t k;                    /* LocalizationPlaneDistanceNbrNeighbors = 5 (LS.h:277); only 5 supported */
  int32_t tukey_variant;        /* 0 = Ceres 2.0.0 TukeyLoss (rho' = 0.5 (1-s/a^2)^2); 1 = Ceres >= 2.1 */
  int32_t time_kernels;         /* HIP-event timing on the context's stream (so_icp_get_timing): 1 = the k-NN kernel only, on every
                                   3rd registration (events attached to the dispatch; cheap enough for a timed region),
                                   2 = every kernel of every registration (adds pipeline bubbles; profiling only) */
  float line_res, plane_res;    /* localMap.lineRes_/planeRes_ (LM.h:760-761; pushed every frame, lmap.cpp:648-649) */
  double yaw_ratio;             /* OptSet.yaw_ratio (LS.cpp:906) */
  double velocity_failure_threshold; /* OptSet.velocity_failure_threshold (LS.cpp:179) */
  int32_t shard_mode;           /* world_size > 1: SO_ICP_SHARD_MAP (0) = the map sharded by brick-hash of the voxel grid, queries follow
                                   their cell's owner (BASELINE configs[3]); SO_ICP_SHARD_QUERIES (1) = the map replicated on every
                                   rank, the scan's 64-point segments dealt round-robin to the ranks -- equal shares whatever the scene,
                                   no halo, no re-binning; the same 45-double exchange per evaluation in both */
  int32_t solve_workgroups;     /* 0 = one workgroup of the persistent solve launch per compute unit (default); n >= 1: at most n -- the
                                   launch needs ALL its workgroups resident at once, so contexts (or ranks) that share a device must
                                   leave each other room: sum of the values <= compute units.  Results do not depend on it beyond the
                                   order of the fp64 sums (SOICP_SOLVE_WORKGROUPS in the environment overrides it: test aid) */
} so_icp_config;
#define SO_ICP_SHARD_MAP 0
#define SO_ICP_SHARD_QUERIES 1

/* super_odometry_msgs/msg/IterationStats.msg + what LS.cpp:242-251 fills + solver summary */
typedef struct {
  double translation_norm, rotation_norm;
  int32_t num_surf_from_scan;   /* accepted correspondences A (planner_num) */
  int32_t num_corner_from_scan; /* always 0: the edge path is dead */
  int32_t lm_iterations;        /* minimizer iterations executed (iteration 0 not counted) */
  int32_t num_successful_steps; /* ceres::Solver::Summary::num_successful_steps (LS.cpp:141) */
  int32_t termination;          /* 0 max-iter, 1 function tol, 2 parameter tol, 3 gradient tol, 4 no residuals, 5 failure */
  int32_t reserved;
  double initial_cost, final_cost;
  int32_t reject_hist[SO_ICP_N_REJECT]; /* MatchRejectionHistogramPlane, LS.cpp:341 */
  int32_t obs_hist[SO_ICP_N_OBS];       /* PlaneFeatureHistogramObs, LS.cpp:336-339 */
  double pose_after[7];
} so_icp_iter_stats;

/* super_odometry_msgs/msg/OptimizationStats.msg: every field the reference fills (LS.cpp:198-210,
 * 242-251, 371-377, 969-974) + the final normal equations (enables EstimateRegistrationError,
 * LS.cpp:854-889, on the caller side without the A x 6 SVD). */
typedef struct {
  int32_t laser_cloud_surf_from_map_num;
  int32_t laser_cloud_corner_from_map_num; /* 0 */
  int32_t laser_cloud_surf_stack_num;
  int32_t laser_cloud_corner_stack_num;    /* 0 */
  int32_t n_iterations;                    /* outer ICP iterations executed */
  int32_t startup_count;                   /* LidarSLAM::startupCount side effect (LS.cpp:181) */
  int32_t pos_in_localmap[3];              /* LS.cpp:363 */
  int32_t prediction_source;               /* LS.cpp:278: reset to 0; 1 when the registration carried a pose prior (:297) */
  double total_translation, total_rotation;
  double translation_from_last, rotation_from_last;
  double time_elapsed_ms;                  /* TicToc over the ICP loop, LS.cpp:118,199-200 */
  double uncertainty[6];                   /* x y z roll pitch yaw, LS.cpp:915-974 (histogram of the previous scan) */
  double JtJ[36], Jtr[6];                  /* loss-corrected normal equations at the returned pose */
  so_icp_iter_stats iterations[SO_ICP_MAX_OUTER];
  uint32_t flags;                          /* SO_ICP_FLAG_*: degraded / non-default modes this registration ran in -- what the
                                              reference would print as a warning (LS.cpp:113-116 style), for the node's log */
  uint32_t reserved;
} so_icp_stats;

/* so_icp_stats::flags */
#define SO_ICP_FLAG_PER_EVAL_LAUNCHES 0x1u   /* the persistent solve launch is not in use (disabled by a failed co-residency
                                                 wait, SOICP_PERSISTENT=0, a sharded map or a concurrent batch): ~2x slower solve */
#define SO_ICP_FLAG_RETRIED 0x2u             /* THIS registration was repeated after an abandoned persistent solve launch */
#define SO_ICP_FLAG_HOST_MAP 0x4u            /* LocalMap lives on the host and is re-uploaded after every insert (planeRes < 0.1
                                                 or SOICP_HOST_MAP=1) */
#define SO_ICP_FLAG_SORT_BINNING 0x8u        /* reserved (the sort-binning path of ABI v2 rounds 1-2 no longer exists; never set) */
#define SO_ICP_FLAG_SHARDED 0x10u            /* world_size > 1: map shard + collective per evaluation */
#define SO_ICP_FLAG_STAGED_SCAN 0x20u        /* the scan came from so_icp_stage_scan (upload overlapped with earlier work) */
#define SO_ICP_FLAG_COPY_READBACK 0x40u      /* state read back with hipMemcpyAsync (SOICP_READBACK=copy) */
#define SO_ICP_FLAG_QUERY_SPLIT 0x80u        /* world_size > 1 with SO_ICP_SHARD_QUERIES: map replicated, this rank registered its share of the scan */
#define SO_ICP_FLAG_BINNED_AHEAD 0x100u      /* the staged scan had been spatially binned behind its copy, beside the registration before it
                                                 (single device; SOICP_PREBIN=0 disables): this registration started with its k-NN sweep */
#define SO_ICP_FLAG_QUERY_WAVES 0x200u       /* small scan (<= 4 096 kept queries, e.g. max_surface_features 2000 / 4000 of the stock configurations): no
                                                 binning, every kept query searched by a wavefront of its own (SOICP_QUERY_WAVES=0 disables): identical results */

#define SO_ICP_FLAG_CHAINED 0x400u           /* so_icp_register_sequence: this registration's launches were enqueued behind the registration before it, before
                                                 that one had reported; its guess (guesses_out) was formed on the device */
#define SO_ICP_FLAG_POSE_PRIOR 0x800u        /* the registration carried the prior of so_icp_set_pose_prior: costs, JtJ and Jtr include it */

/* average kernel durations since the last so_icp_reset_timing (HIP events on the context's stream) */
typedef struct {
  double knn_ms_total;   int64_t knn_launches;   int64_t knn_queries;   int64_t knn_map_points;
  double eval_ms_total;  int64_t eval_launches;  int64_t eval_points;
  double prep_ms_total;  int64_t prep_launches;
  double host_ms_total;  int64_t registrations;
  /* k-NN kernel statistics (time_kernels only): wave group passes, lanes sent to the exact per-lane scan,
   * wave-uniform candidates streamed */
  int64_t knn_group_passes, knn_fallback_lanes, knn_candidates_scanned;
  /* so_icp_stage_scan: host time registrations spent waiting for a staged scan that was still on its way through the copy
   * thread; announcements copied by DMA straight from registered host memory / through the copy thread / declined */
  double stage_wait_ms_total;  int64_t staged_direct, staged_copied, stage_declined;
  /* packed light chunks of the k-NN sweep (time_kernels 2 + SOICP_ABLATE only): rows of 16 lanes with work, rows left to the
   * group passes because their block has more than 16 x-runs / keeps more than its quarter of the tile, candidates kept */
  int64_t knn_packed_rows, knn_packed_rows_too_many_runs, knn_packed_rows_tile_full, knn_packed_kept;
  /* host adaptivity of the packing (every registration counts): registrations whose sweeps packed their light chunks, and how
   * often a registration that left > 3 % of its queries to the exact scan switched the packing off for the next 32 */
  int64_t knn_pack_registrations, knn_pack_holds;
  /* so_icp_register_sequence: registrations whose launches were enqueued behind the registration before them (SO_ICP_FLAG_CHAINED), and how
   * often a registration needed more outer iterations than were enqueued ahead (the chained registration behind it then started again) */
  int64_t seq_chained, seq_chain_breaks;
} so_icp_timing;

/* -------- lifecycle ------------------------------------------------------------------------ */
void so_icp_default_config(so_icp_config *cfg);
so_icp_ctx *so_icp_create(const so_icp_config *cfg); /* NULL on failure: see so_icp_last_error(NULL) */
void so_icp_destroy(so_icp_ctx *ctx);
const char *so_icp_last_error(const so_icp_ctx *ctx); /* ctx may be NULL for creation errors */
int so_icp_abi_version(void);
/* 1 when a HIP device is usable by this library; the product has NO CPU fallback */
int so_icp_device_available(void);
/* HIP devices visible to this process (one process per GPU: device_id = LOCAL_RANK) */
int so_icp_device_count(void);

/* -------- per-frame knobs (public fields the node writes, lmap.cpp:648-649, 703-711) ---------- */
/* planeRes may change between frames (auto_voxel_size, lmap.cpp:604-649): the resident points stay as they are, the index
 * follows, the next insert re-filters the cubes it touches (LM.h:617-641).  world_size > 1: the shards are cut along the
 * cell grid, which follows planeRes, so a CHANGE of planeRes over a non-empty map re-cuts them from every rank's points --
 * a COLLECTIVE step over the communicator (every rank makes the same call; all-gather of the owned points, a few MB);
 * without a communicator the change is refused with SO_ICP_E_UNSUPPORTED. */
int so_icp_set_resolution(so_icp_ctx *ctx, float line_res, float plane_res);
int so_icp_set_max_surface_features(so_icp_ctx *ctx, int max_surface_features);
int so_icp_set_max_iterations(so_icp_ctx *ctx, int max_iterations);
/* The surf cloud's INTENSITY through pre-filter, map insert and map export.  In the reference the surf cloud is pcl::PointXYZI, its
 * intensity the point's sweep-relative time (featureExtraction.cpp:513), and the field survives the whole path: adjustVoxelSize's
 * pcl::VoxelGrid<PointXYZI> averages every field per leaf (downsample_all_data, PCL's default; laserMapping.cpp:639-645),
 * transformAndAddToMap copies the point and rewrites x y z only (LidarSlam.cpp:69-71, superodom_utils.h:126-130),
 * LocalMap::addSurfPointCloud runs the same VoxelGrid over every touched cube (LocalMap.h:621-627), and publishTopic sends the map
 * clouds through pcl::toROSMsg, 32 bytes per point as they are (laserMapping.cpp:437-456).
 * offset_bytes: -1 (the state of a new context) = off: every entry point gives the bytes it gave without this call.  Otherwise the
 * byte offset of a FLOAT32 intensity inside a point record, 16 for pcl::PointXYZI; < 12 or not a multiple of 4: SO_ICP_E_INVALID.
 * A host-only context, one on the host-side map (SOICP_HOST_MAP=1, plane_res < 0.05) or world_size > 1: SO_ICP_E_UNSUPPORTED.
 * The switch may change between calls; points in the map keep the intensity they have.  While it is on:
 *  - so_icp_map_add_surf, so_icp_localization (seeding and register + insert; staged with so_icp_stage_scan or not: the same map; and
 *    so_icp_localization_sequence on host scans, which runs it) and so_icp_prefilter_scan(_dev) read a point's intensity at
 *    offset_bytes when stride_bytes >= offset_bytes + 4; else the point's intensity is 0.
 *  - so_icp_localization_dev inserts with the pre-filter's intensities when called with exactly the last pre-filter's *d_filtered_out
 *    and *n_out; any other resident scan inserts intensity 0.
 *  - so_icp_map_export_records writes 1.0f at byte 12 (stride_bytes >= 16: data[3] of the PointXYZI constructor) and the intensity at
 *    byte 16 (stride_bytes >= 20).  so_icp_map_export and every registration entry are unaffected.
 * Rules (pcl::CentroidPoint<PointXYZI>: AccumulatorXYZ a Vector3f sum, AccumulatorIntensity a float sum, both divided by the count as
 * float; PCL is not part of this project's test oracle, the rules are restated like the x y z centroid's): a leaf's intensity is the
 * sequential float sum of its members' intensities in the member order of the x y z sums -- old centroids of the cube first, then the
 * new points in scan order -- divided by (float)count; a lone point keeps its intensity.  Intensity is data: no cube, leaf, cell,
 * order, gate or count depends on it, and a NaN or infinite one makes its leaf's intensity non-finite and changes nothing else. */
int so_icp_set_cloud_intensity(so_icp_ctx *ctx, int offset_bytes);

/* -------- LocalMap (LM.h) ------------------------------------------------------------------ */
int so_icp_map_set_origin(so_icp_ctx *ctx, const double t_w_cur[3], int origin_out[3]); /* LocalMap::setOrigin, LM.h:146-164 */
int so_icp_map_shift(so_icp_ctx *ctx, const double t_w_cur[3], int pos_in_map[3]);      /* LocalMap::shiftMap,  LM.h:169-287 */
/* LocalMap::addSurfPointCloud, LM.h:591-645: world-frame points (stride in bytes, 12 for packed xyz,
 * 32 for pcl::PointXYZI); bins into 50 m cubes, VoxelGrid(planeRes) per touched cube, rebuilds the
 * device index.  Returns the number of points that fell inside the 21x21x11 window, or <0.
 * world_size > 1: every rank passes the SAME cloud and keeps its shard of it; with a communicator (RCCL or in-process
 * group) the call is collective -- the per-block point counts of the full map are summed over the ranks. */
int so_icp_map_add_surf(so_icp_ctx *ctx, const float *xyz, size_t n, size_t stride_bytes);
int so_icp_map_count_5x5(so_icp_ctx *ctx, const int pos[3], int *n_edge, int *n_surf);  /* get5x5LocalMapFeatureSize, LM.h:292-318 */
/* getAllLocalMap / get5x5LocalMap (LM.h:646-688): points in the canonical (device) order */
int so_icp_map_export(so_icp_ctx *ctx, float *xyz, size_t cap_points, size_t *n_out, int only_5x5, const int pos[3]);
/* The same points as RECORDS of stride_bytes (float x, y, z first, the remaining bytes zero; with so_icp_set_cloud_intensity on, 1.0f at
 * byte 12 and the intensity at byte 16 -- stride 32: the pcl::PointXYZI pcl::toROSMsg puts into the laser_cloud_map / laser_cloud_surround messages, lmap.cpp:437-462), written straight to `out`: the
 * payload area of the message being assembled.  One gather, one copy (DMA when `out` lies in so_icp_host_alloc / _register memory), one
 * synchronisation -- so_icp_map_export makes a round trip per occupied cube.  out == NULL (or more points than cap_points): the count only. */
int so_icp_map_export_records(so_icp_ctx *ctx, void *out, size_t stride_bytes, size_t cap_points, size_t *n_out, int only_5x5, const int pos[3]);
int so_icp_map_size(so_icp_ctx *ctx, size_t *n_points, size_t *n_points_this_rank);
int so_icp_map_clear(so_icp_ctx *ctx);
int so_icp_map_get_origin(so_icp_ctx *ctx, int origin_out[3]);
/* Diagnostics of the device-resident map's insert (LM.h:591-645 on the device): how many inserts the device laid out itself
 * -- touched cubes, slots and counts worked out by the insert's first kernel, no read-back -- and how many of those it had
 * to hand back to the host (a cube without a slot, more cubes than a round holds, a cube that needs the sort).  Both 0
 * with the host-side map (world_size > 1) or SOICP_MAP_FAST=0. */
int so_icp_map_insert_stats(so_icp_ctx *ctx, unsigned *device_built, unsigned *handed_back);

/* -------- Seam B: LocalMap::nearestKSearchSurf (LM.h:481-525), batched ------------------------ */
/* Host buffers. found[i]=0 reproduces the `return false` paths (cube outside the window, LM.h:499-502,
 * or no tree, LM.h:506).  Unfilled slots reproduce nanoflann.h:87-100 (idx 0 -> first point of the cube,
 * d2 = 0 except d2[k-1] = FLT_MAX). Exact cube-restricted k-NN; ties by ascending canonical index. */
int so_icp_knn_surf(so_icp_ctx *ctx, const float *q_xyz, size_t nq, int k,
                    float *nbr_xyz /* nq*k*3 */, float *d2 /* nq*k */, int32_t *nbr_index /* nq*k, nullable */,
                    uint8_t *found /* nq */);

/* -------- Seam A: LidarSLAM::performLocalizationAndMapping (LS.cpp:107-152 + 155-210) --------- */
/* scan: sensor frame, already voxel-filtered by the node (lmap.cpp:643-645).  Does shiftMap,
 * the <=50-feature check, the outer ICP loop and the post-processing statistics; does NOT insert
 * the scan into the map (so_icp_localization does).  prev uncertainty comes from the previous call. */
int so_icp_register(so_icp_ctx *ctx, const float *scan_xyz, size_t n, size_t stride_bytes,
                    const double pose_in[7], double pose_out[7], so_icp_stats *stats);
/* A RUN of scans whose guesses chain (a node working off a backlog of feature clouds in localization mode; a log replayed at full
 * speed): guess_0 = pose0, guess_k = T_(k-1) o delta_k -- T_(k-1) the pose registration k-1 ended with, delta_k the motion prediction
 * between the two scans in the sensor frame: what laserMapping::selectPosePrediction (lmap.cpp:345-372) does with the LIO / VIO /
 * IMU predictions, `T_w_lidar = T_w_lidar * prediction` (Twist::operator*, utils/Twist.h:181-185): t = t + R(q) dt, q = normalize(q dq).
 * Equivalent to `count` calls of so_icp_register (so_icp_register_dev with scans_on_device) from guesses_out[k], bit for bit.  What it
 * buys: the launches of registration k+1 are enqueued BEHIND those of registration k before k has reported -- the guess is formed on
 * the device --, so the device does not idle for the host's turn-around between two calls (~11 us of a 140 us registration), and
 * scan k+1 is copied and binned beside registration k under the predicted guess.  A registration that turns out to need more outer
 * iterations than were enqueued ahead is finished the ordinary way and the one behind it starts again (so_icp_timing::seq_chain_breaks).
 * The map is NOT updated in between: the whole run is registered against a fixed (prior) map -- an extension for replay, not the reference's
 * loop, which inserts every registered frame (LidarSlam.cpp:154-167; `localization_mode` only chooses the prior map and the start pose,
 * laserMapping.cpp:163-173, 306).  so_icp_localization_sequence below runs the reference's register-then-insert order.
 * scans[k]: host pointers (packed or strided xyz; memory from so_icp_host_alloc / so_icp_host_register is copied by DMA) or, with
 * scans_on_device, device pointers to packed xyz.  deltas: count x 7 {dx, dy, dz, qx, qy, qz, qw}, row 0 unused.  poses_out: count x 7;
 * guesses_out (count x 7, nullable): the guess each registration started from; stats (count, nullable); n_done (nullable): registrations
 * completed -- on an error or SO_ICP_NOT_ENOUGH_MAP_FEATURES the run stops at that scan and its code is returned.
 * The chained path needs a single device, the device-resident map and yaw_ratio 0 (every stock configuration: MannualYawCorrection,
 * LS.cpp:891-913, is then the identity up to rounding, and the chain continues from the optimised pose itself,
 * stats[k].iterations[last].pose_after); otherwise -- or with SOICP_SEQ_CHAIN=0 -- the registrations run one after the other, same results. */
int so_icp_register_sequence(so_icp_ctx *ctx, int count, const void *const *scans, const size_t *n_points, size_t stride_bytes,
                             int scans_on_device, const double pose0[7], const double *deltas, double *poses_out, double *guesses_out,
                             so_icp_stats *stats, int *n_done);
/* A run of frames in the reference's per-frame order (LidarSlam.cpp:30-51, 107-167): for k = 0..count-1
 *   guess_k = (k == 0 ? pose0 : pose_out_(k-1) o delta_k); register scan k from guess_k (as so_icp_localization);
 *   checkMotionThresholds bookkeeping with times[k]; insert T_k * scan_k into the map (transformAndAddToMap).
 * Equivalent, bit for bit, to `count` so_icp_localization(_dev) calls (initialization = 1) from guesses_out[k],
 * including the map after every frame.  The map must already be seeded.  Returns like so_icp_register_sequence
 * (first error / SO_ICP_NOT_ENOUGH_MAP_FEATURES stops the run at that frame; *n_done frames were registered AND inserted).
 * Unlike so_icp_register_sequence the chain continues from pose_out_(k-1), the pose AFTER MannualYawCorrection (LidarSlam.cpp:891-913),
 * as the node does (`T_w_lidar = T_w_lidar * prediction`, laserMapping.cpp:345-372); so_icp_register_sequence continues from the
 * optimised pose before it.  An extension for replaying a log or building a map offline: the reference node drops a backlog
 * (clearSensorData, laserMapping.cpp:689-699).  times: count stamps (time_laser_odometry of each frame); the other arguments as for
 * so_icp_register_sequence.  A convenience entry: the frames run one after the other through the per-frame entry points (registration
 * k + 1 is NOT enqueued before the host has read frame k's report: the insert of k needs the host's pose_out_k), so it takes as long
 * as the caller's own loop.
 * A host-only context fails with SO_ICP_E_HIP before touching its map; count == 0 does nothing. */
int so_icp_localization_sequence(so_icp_ctx *ctx, int count, const void *const *scans, const size_t *n_points,
                                 size_t stride_bytes, int scans_on_device, const double pose0[7], const double *deltas,
                                 const double *times, double *poses_out, double *guesses_out, so_icp_stats *stats, int *n_done);
/* A backlog worked off in several calls: name the scan that will START the next so_icp_register_sequence call (packed xyz in host memory,
 * n points) and the motion prediction from the LAST scan of the coming call to it.  That call then copies and bins it beside its last
 * registration, and the call after it -- whose scans[0] is this very buffer -- starts with its first sweep instead of a copy and a binning
 * nothing hides (55 us for a 131 072-point scan).  The buffer must stay valid and unchanged until that second call returns; scan == NULL
 * withdraws the announcement (and waits for a copy already under way).  Results never depend on it. */
int so_icp_sequence_announce_next(so_icp_ctx *ctx, const float *scan_xyz, size_t n, const double delta[7]);
/* Announce the NEXT scan: the host buffer travels to HBM on the context's copy stream while the caller goes on (typically:
 * while the previous so_icp_register is still running -- the node's feature callback, lmap.cpp:21-25, has the cloud long
 * before process() reaches it).  Packed xyz (stride 12) inside a buffer pinned with so_icp_host_register is read by DMA
 * straight from the caller's memory: this call enqueues the copy and returns, and the registration's first kernel waits for
 * it on the device.  Anything else (pageable memory, strided pcl::PointXYZI records) is packed into a pinned buffer by the
 * context's copy thread first.  A following so_icp_register / so_icp_localization with the SAME (scan_xyz, n, stride_bytes)
 * consumes the staged copy instead of uploading again (so_icp_stats::flags carries SO_ICP_FLAG_STAGED_SCAN); any other call
 * simply ignores it.  The caller's buffer must stay valid and unchanged until that call returns (a DMA copy reads it when the
 * registration in flight has its first launch in the queue, or 300 us after the announcement, whichever comes first); to take a
 * staged buffer back without registering it, announce it again (the older copy is superseded) or call so_icp_stage_cancel.
 * A DMA copy that a registration in flight enqueues is followed, on the copy stream, by the scan's spatial binning under that
 * registration's guess (single device, device-resident map): the consuming registration then starts with its k-NN sweep
 * (SO_ICP_FLAG_BINNED_AHEAD).  The binning only groups queries for the sweep -- results do not depend on it.
 * Three slots: two scans may be announced ahead of the one being registered; a further announcement returns
 * SO_ICP_STAGE_DECLINED (soft: that scan is uploaded by its own registration call).  Announcing a buffer again supersedes
 * its earlier copy; a copy announced BEFORE a scan that has been consumed since (a skipped frame) is never served and gives
 * its slot to the next announcement.  A staged copy is also dropped by a map-seeding so_icp_localization(initialization = 0)
 * on the same buffer.  Unlike the other entry points this one may be called from ANOTHER thread than the registration calls
 * (the node's feature callback, lmap.cpp:21-25). */
int so_icp_stage_scan(so_icp_ctx *ctx, const float *scan_xyz, size_t n, size_t stride_bytes);
/* withdraw every staged copy of this host buffer (returns when nothing reads the buffer any more) */
int so_icp_stage_cancel(so_icp_ctx *ctx, const float *scan_xyz);
/* Pin a host buffer the caller keeps its clouds in (hipHostRegister; the node's copy of the message payload into its feature
 * cloud, pcl::fromROSMsg at lmap.cpp:250-263, then lands in pinned memory): so_icp_stage_scan and so_icp_register copy
 * packed scans that lie inside it by DMA without an intermediate copy.  Unregister before freeing the buffer. */
int so_icp_host_register(so_icp_ctx *ctx, const void *ptr, size_t bytes);
int so_icp_host_unregister(so_icp_ctx *ctx, const void *ptr);
/* Pinned host memory from the HIP runtime's allocator (hipHostMalloc), owned by the context until so_icp_host_free /
 * so_icp_destroy: a pool for the caller's clouds without a registration call per buffer. */
int so_icp_host_alloc(so_icp_ctx *ctx, size_t bytes, void **ptr_out);
int so_icp_host_free(so_icp_ctx *ctx, void *ptr);
/* same, scan already resident in HBM as packed float xyz (n*3 floats, device pointer) */
int so_icp_register_dev(so_icp_ctx *ctx, const void *d_scan_xyz, size_t n,
                        const double pose_in[7], double pose_out[7], so_icp_stats *stats);
/* Batched hypotheses (BASELINE.json configs[4], the "degeneracy / alignment-risk" use): the SAME scan registered from
 * n_hyp initial poses (poses_in = n_hyp x 7).  Every hypothesis is an independent so_icp_register (own binning, own
 * correspondences, own LM solves); the map window is shifted once, for hypothesis 0 (LS.cpp:363), and the context's
 * scan-to-scan state (previous observability histogram, startup counter) is left as it was.  Groups of up to 64
 * hypotheses go through batched kernels -- one binning / k-NN / persistent-solve launch per outer iteration over all
 * hypotheses still running, a group of workgroups and an LM controller per hypothesis -- whose sums follow the summation
 * tree of the single registration: results are bit-identical to one so_icp_register per hypothesis.  A device that cannot
 * keep the batched solve resident falls back by itself (one workgroup per compute unit, then concurrent sequential
 * registrations on worker contexts that borrow this context's resident map); same bits.  d_scan_xyz != NULL
 * takes a scan already resident in HBM (so_icp_upload_scan), else scan_xyz is uploaded once.  Returns the number of
 * hypotheses that returned SO_ICP_OK (>= 0), or a negative error; rc_out[h] (nullable) = status of hypothesis h.
 * so_icp_set_batch_priors (below) gives every hypothesis of the next call a pose prior of its own; that call consumes them, and a
 * call whose n_hyp differs from theirs returns SO_ICP_E_INVALID and leaves them pending. */
int so_icp_register_batch(so_icp_ctx *ctx, const float *scan_xyz, const void *d_scan_xyz, size_t n, size_t stride_bytes,
                          const double *poses_in, int n_hyp, double *poses_out, so_icp_stats *stats /* n_hyp, nullable */,
                          int32_t *rc_out /* n_hyp, nullable */);

/* LidarSLAM::EstimateRegistrationError (LS.cpp:854-889) from the final normal equations in so_icp_stats, without the
 * A x 6 SVD: covariance in the tangent space = (J^T J)^-1 with the loss applied (ceres::Covariance,
 * apply_loss_function = true, GetCovarianceBlockInTangentSpace), then the eigen-analysis of its position and
 * orientation blocks (LS.h:127-151).  Host arithmetic only; returns SO_ICP_E_INVALID when J^T J is singular. */
typedef struct {
  double covariance[36];               /* row-major, DoF order X Y Z rX rY rZ */
  double position_error;               /* sqrt(largest eigenvalue of the position block) */
  double position_error_direction[3];
  double pos_inverse_condition_num;    /* sqrt(lambda_min) / sqrt(lambda_max) */
  double orientation_error_deg;        /* Rad2Deg(sqrt(largest eigenvalue of the orientation block)) */
  double orientation_error_direction[3];
  double ori_inverse_condition_num;
} so_icp_registration_error_t;
int so_icp_registration_error(const so_icp_stats *stats, so_icp_registration_error_t *out);

/* upload a scan once and keep it resident in HBM (device pointer owned by the context until
 * so_icp_free_scan / so_icp_destroy) */
int so_icp_upload_scan(so_icp_ctx *ctx, const float *scan_xyz, size_t n, size_t stride_bytes, void **d_scan_out);
int so_icp_free_scan(so_icp_ctx *ctx, void *d_scan);

/* LidarSLAM::Localization (LS.cpp:30-51): initialization==0 seeds the map (LS.cpp:83-94) and returns
 * SO_ICP_MAP_SEEDED; otherwise registers, applies the post-processing and inserts the scan
 * (transformAndAddToMap, LS.cpp:60-80, 163-167). */
int so_icp_localization(so_icp_ctx *ctx, int initialization, const double T_w_lidar[7],
                        const float *planar_xyz, size_t n, size_t stride_bytes, double time_laser_odometry,
                        double pose_out[7], so_icp_stats *stats);

/* same, scan already resident in HBM as packed float xyz (e.g. the output of so_icp_prefilter_scan) */
int so_icp_localization_dev(so_icp_ctx *ctx, int initialization, const double T_w_lidar[7], const void *d_scan_xyz, size_t n,
                            double time_laser_odometry, double pose_out[7], so_icp_stats *stats);
/* copy a resident scan (packed float xyz) back to the host */
int so_icp_download_scan(so_icp_ctx *ctx, const void *d_scan_xyz, size_t n, float *out_xyz);

/* -------- what Seam A leaves behind: the CORRESPONDENCE SET of the last registration -- the reference's features_corres
 * (tbb::concurrent_vector<OptimizationParameter>, LS.h:209-222), filled by extractFeaturesConstraints (LS.cpp:299-344) on every outer
 * iteration: per scan point the MatchingResult, and per accepted point the plane (NormDir, negative_OA_dot_norm) and the
 * residualCoefficient.  The registration already stores all of it in memory of the context; this entry reads it there (one launch of
 * a kernel of its own; no registration kernel takes part and none was changed for it).  What a caller does with it: colour or mask the
 * registered scan by residual, keep points that matched nothing out of the map, hand a factor-graph back end point-to-plane factors
 * instead of one pose, re-evaluate the cost of the fixed set at another pose.
 * The hypotheses of so_icp_register_batch: so_icp_keep_batch_correspondences and so_icp_batch_correspondences, far below; EVERY frame of
 * a run of so_icp_register_sequence / so_icp_localization_sequence: so_icp_keep_sequence_correspondences, behind them.  Not exported:
 * the correspondences of a sharded context (world_size > 1).  The
 * neighbours, the PCA and the observability labels of every accepted point: so_icp_correspondence_geometry, below.  Normal
 * equations: so_icp_stats::JtJ / Jtr are those of the set at the default pose; at other poses so_icp_correspondence_sums (below, with so_icp_match) sums them on the device -- or the caller
 * sums them from the records: J = [n, p x (R^T n)], JtJ += weight J J^T, Jtr += weight residual J. */
/* One accepted correspondence of the last outer iteration (LS.h:209-222: Xvalue, NormDir, negative_OA_dot_norm,
 * residualCoefficient), plus its residual and weight at the evaluation pose. */
typedef struct {
  uint32_t index;   /* position of the point in the scan */
  float p[3];       /* the scan point, sensor frame, the scan's own bits */
  double n[3];      /* NormDir */
  double d;         /* negative_OA_dot_norm */
  double coeff;     /* residualCoefficient */
  double residual;  /* n . (R(q) p + t) + d at pose_eval (lidarOptimization.cpp:59-61) */
  double weight;    /* coeff * rho'(residual^2): this row's factor in J^T J and J^T r */
} so_icp_correspondence;   /* 72 bytes */
typedef struct {
  uint64_t n_points, n_accepted;
  int32_t valid;            /* 0: nothing to export (below); every count 0 */
  int32_t outer_iteration;  /* = so_icp_stats::n_iterations - 1 of that registration */
  double pose_fit[7];       /* the pose the correspondences were formed at: the registration's guess when n_iterations == 1 (in a chained
                               sequence guesses_out[k]), else iterations[n_iterations - 2].pose_after */
  double pose_eval[7];      /* the pose residual, weight and cost are evaluated at */
  double cost;              /* sum 0.5 * coeff * rho(residual^2) over the records: Ceres' cost of the set at pose_eval */
} so_icp_correspondence_info;
/* The switch.  A new context has it off, and while it is off every entry does exactly what it does without this feature (no launch,
 * copy, allocation or synchronisation is added) and so_icp_correspondences reports valid = 0.  While it is on, every registration that
 * ends with SO_ICP_OK -- so_icp_register, _register_dev, so_icp_localization(_dev) with initialization = 1, the last registration of
 * so_icp_register_sequence, the last frame of so_icp_localization_sequence -- leaves what the export needs in memory the context owns
 * (of a run only the LAST frame: the arrays are the context's own, and the frames behind a frame overwrite them; the sets of ALL frames
 * are kept under a switch of their own, so_icp_keep_sequence_correspondences, far below).
 * The records and status bytes are there anyway; the SCAN is not (it may lie in a stage slot that so_icp_stage_scan refills from another
 * thread as soon as the call returns, in the caller's device buffer, or in the pre-filter's output), so the registration keeps a
 * packed copy of it: one device-to-device copy of 12 n bytes in the context's queue, in front of the registration's first launch (a
 * staged scan has arrived by then and its slot is released only after the registration has reported, which is behind the copy); the
 * last registration of a CHAINED so_icp_register_sequence copies behind its report and waits for the copy.
 * Turning the switch off drops the set.  world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP. */
int so_icp_keep_correspondences(so_icp_ctx *ctx, int on);
/* The set of the last registration.  info->valid = 0 (SO_ICP_OK, every count 0, no output touched) when the switch was off during the
 * last registration, there has been none, the last registration-family call returned anything but SO_ICP_OK
 * (SO_ICP_NOT_ENOUGH_MAP_FEATURES, SO_ICP_MAP_SEEDED, an error) or was so_icp_register_batch.  Nothing else invalidates it: not the map
 * insert of so_icp_localization, not a pre-filter, not a staged announcement, not so_icp_knn_surf.
 * pose (nullable): where residual, weight and cost are evaluated; NULL = stats.iterations[n_iterations - 1].pose_after, the optimised
 * pose BEFORE MannualYawCorrection (LS.cpp:891-913), where so_icp_stats::JtJ / Jtr were formed.  The arithmetic is the solve's own
 * (quat_rotate in fp64, + t, the fused dot product, s = r^2 against a^2, v = 1 - s (1 / a^2), rho' = 0.5 v^2 (tukey_variant 0) or v^2 (1),
 * 0 outside the window; rho = rho_out (1 - v^3) inside, rho_out = a^2 / 6 or a^2 / 3 outside), with the a^2 and the variant of THAT
 * registration: a later so_icp_set_resolution does not change them.  At the default pose the records carry the residuals and weights
 * of the registration's last evaluation, and cost its final_cost up to the order of the sum; at pose_fit, its initial_cost.
 * Outputs, each nullable:
 *  records     the accepted correspondences (status 0) in ascending index; NULL or cap_records < n_accepted: the counts only
 *  status_out  [i] = the MatchingResult byte of point i, 254 = not sampled (what so_icp_debug_match_status gives)
 *  residual_out[i] = (float)residual of an accepted point, NaN otherwise; both per-point arrays need cap_points >= n_points
 *                    (SO_ICP_E_INVALID otherwise)
 *  *d_records_out  a device buffer owned by the context with the same record bytes, valid until the next so_icp_correspondences
 *                  call; no other entry writes it
 * cost is a deterministic sum (per-tile partial sums in a fixed tree, the tiles added in tile order): two calls give the same bits.
 * One launch, one copy per requested host output (and one of the counts and tile sums), one synchronisation, on the context's queue
 * behind whatever the last call left there.  A registered scan of 0 points: valid = 1, zero counts.  SO_ICP_E_UNSUPPORTED for a scan
 * of 2^31 points or more (the registration entries refuse far smaller ones). */
int so_icp_correspondences(so_icp_ctx *ctx, const double pose[7] /* nullable */,
                           so_icp_correspondence *records, size_t cap_records,
                           uint8_t *status_out, float *residual_out, size_t cap_points,
                           void **d_records_out, so_icp_correspondence_info *info);

/* -------- the GEOMETRY of the kept set: what the reference keeps of pcaFeature inside OptimizationParameter (LS.h:209-222) and what
 * FeatureObservabilityAnalysis (LS.cpp:574-693) labels -- per accepted point the five neighbours it matched, the eigenvalues of their
 * scatter, the PCA normal, the mean plane distance and the three observability labels that fill obs_hist (and so
 * so_icp_stats::uncertainty, LS.cpp:289-291).  The registration does not store these; it SNAPSHOTS, behind the launch that produced
 * its final report and in front of anything that can change the map (so_icp_localization's insert included), the five neighbour
 * indices of every accepted point and the five map points they name -- the bits its last fit pass read -- into memory the context
 * owns (one launch on the context's queue, 81 bytes per scan point).  The export refits from the snapshot with the fit pass's own
 * code (plane_fit.h), so it depends on nothing a later call can change: not so_icp_map_add_surf, so_icp_map_shift,
 * so_icp_set_resolution, a pre-filter or a staged announcement. */
typedef struct {
  uint32_t index;          /* position in the scan; record j pairs with record j of so_icp_correspondences */
  uint32_t nbr_index[5];   /* canonical map indices AT THE TIME of the registration, nearest first (ties: ascending index) */
  uint8_t  obs[3];         /* the three labels obs_hist counts: rotation #1, rotation #2, translation #1 (LS.cpp:336-339) */
  uint8_t  reserved;
  float    nbr[15];        /* the five neighbours, world frame, the map's own bits */
  float    d2[5];          /* flann/octree.h:93-102 arithmetic, from the float query (float)(R(q) p + t) */
  uint32_t pad;
  double   pw[3];          /* the point at pose_fit, as the fit pass forms it */
  double   eig[3];         /* ascending eigenvalues of the scatter S = sum (x-mu)(x-mu)^T  (not / N) */
  double   pca_normal[3];  /* eigenvector of eig[0], flipped so that pca_normal . pw >= 0 (LS.cpp:553-561) */
  double   mean_abs_dist;  /* the reference's "meanSquareDist": mean |n.p_j + d| (LS.cpp:792-844) */
} so_icp_correspondence_geometry_record;   /* 192 bytes */
/* (the record type carries the suffix _record: C has one namespace for typedefs and functions, and so_icp_correspondence_geometry is
 *  the entry below) */
typedef struct {
  uint64_t n_points, n_accepted;
  int32_t  valid, outer_iteration;   /* as in so_icp_correspondence_info */
  double   pose_fit[7];
  int32_t  obs_hist[9];    /* summed on the device from the records' labels (integer adds): iterations[last].obs_hist */
  int32_t  reserved;
} so_icp_correspondence_geometry_info;
/* The switch.  A new context has it off; while it is off no entry gains a launch, copy, allocation or synchronisation and the export
 * reports valid = 0.  It needs so_icp_keep_correspondences(ctx, 1) (SO_ICP_E_INVALID otherwise), and turning that switch off turns
 * this one off too.  While it is on, every call that leaves a kept set -- so_icp_register, _register_dev, so_icp_localization(_dev)
 * with initialization = 1, the last registration of so_icp_register_sequence, the last frame of so_icp_localization_sequence,
 * so_icp_match(_dev) -- also leaves the snapshot.  world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP. */
int so_icp_keep_correspondence_geometry(so_icp_ctx *ctx, int on);
/* The geometry of the kept set.  info->valid = 0 (SO_ICP_OK, every count 0, no output touched) in exactly the cases of
 * so_icp_correspondences, and when this switch was off during the call that left the set.  Outputs, each nullable:
 *  records     one per accepted point, ascending index; NULL or cap_records < n_accepted: the counts (and obs_hist) only
 *  labels_out  [3 i .. 3 i + 2] = the labels of point i, 255 255 255 where its status is not 0; needs cap_points >= n_points
 *              (SO_ICP_E_INVALID otherwise)
 *  *d_records_out  a device buffer owned by the context with the same record bytes, valid until the next call of this entry; no
 *                  other entry writes it
 * Two calls return identical bytes.  One launch, one copy per requested host output and one of the counts, one synchronisation, on
 * the context's queue.  A registered scan of 0 points: valid = 1, zero counts. */
int so_icp_correspondence_geometry(so_icp_ctx *ctx, so_icp_correspondence_geometry_record *records, size_t cap_records,
                                   uint8_t *labels_out, size_t cap_points,
                                   void **d_records_out, so_icp_correspondence_geometry_info *info);

/* -------- the step before Seam A: laserMapping::adjustVoxelSize (lmap.cpp:598-651) on the device ----------------
 * auto_voxel_size != 0: average_distance = mean|x| * mean|y| * mean|z| of the surf cloud chooses the resolutions
 * (< 25: 0.1 / 0.2, > 65: 0.4 / 0.8, else unchanged), count_far_points (> 3 m) > 3000 raises increase_blind_radius.
 * The choice is ALWAYS the reference's: it accumulates the three sums in float in input order (lmap.cpp:604-611), the device
 * in an fp64 tree; when the statistic is within the reach of those roundings of a threshold, the reference's accumulation
 * itself is run (so_icp_prefilter_info::statistic_in_input_order).
 * Then pcl::VoxelGrid (leaf = planeRes: float leaf coordinates, centroids accumulated in float in input order, output in
 * ascending leaf index; "leaf size too small" passes the cloud through) and localMap.lineRes_/planeRes_ = the result
 * (lmap.cpp:648-649).  *d_filtered_out (packed float xyz, owned by the context, valid until the next call) feeds
 * so_icp_register_dev / so_icp_localization_dev without a host round trip.
 * One enqueue, one read-back: the statistics are reduced, the resolution chosen and the leaf grid laid out on the device
 * (only a statistic inside the rounding band of a threshold, or PCL's "leaf size too small" pass-through, goes through the
 * host); the call runs on a queue of its own, beside the map insert the previous so_icp_localization left in the
 * context's queue, and returns when the filtered cloud is complete. */
typedef struct {
  double average_distance;
  int32_t count_far_points, increase_blind_radius;
  float line_res, plane_res;  /* resolutions in effect after the call */
  int32_t statistic_in_input_order; /* 1: average_distance is the reference's own float accumulation in input order, bit for bit
                                       (taken whenever the value is close enough to 25 / 65 for its roundings to decide);
                                       0: mean|x| mean|y| mean|z| from exact sums -- within 3 n 2^-24 of it, same decision */
  int32_t reserved;                 /* 1: the cloud had been announced (so_icp_prefilter_announce): no copy on this call's path */
} so_icp_prefilter_info;
int so_icp_prefilter_scan(so_icp_ctx *ctx, const float *surf_xyz, size_t n, size_t stride_bytes, int auto_voxel_size,
                          float line_res, float plane_res, void **d_filtered_out, size_t *n_out, so_icp_prefilter_info *info);
/* Announce the NEXT raw surf cloud (laserFeatureInfoHandler has it long before process() reaches it, lmap.cpp:250-263, 768-793): its H2D copy
 * (34 us for a 131 072-point sweep over PCIe) goes into the pre-filter's queue now, beside the registration of the frame before, and the
 * so_icp_prefilter_scan call that names the same buffer (pointer, n, stride) starts with its first kernel; so_icp_prefilter_info::reserved
 * says 1 when that happened.  The buffer must stay valid and unchanged until that call returns; xyz == NULL withdraws the announcement
 * (and waits for a copy under way).  One announcement at a time (a second one replaces the first); any thread.  Results never depend on it. */
int so_icp_prefilter_announce(so_icp_ctx *ctx, const float *surf_xyz, size_t n, size_t stride_bytes);

/* -------- two steps before Seam A: featureExtraction::removePointDistortion
 * (src/FeatureExtraction/featureExtraction.cpp:223-314) on the device.  Every finite point of the sweep is moved to the
 * sensor frame of the sweep start: pose buffer (IMU orientations or VIO odometry, strictly increasing times: the
 * reference keeps them in a std::map) interpolated at lidar_start_time + point.time (slerp / lerp between the two
 * neighbours, the first pose before the buffer starts), T_final = T_w_original^-1 * T_w_current, wrapped in
 * T_l_i * . * T_i_l when the buffer is the IMU's (then positions are ignored: :231-235).  Records: float x y z at byte
 * 0 4 8, float time at time_offset_bytes (point_os::PointcloudXYZITR: stride 32, time at 20); rewritten in place.
 * A point stamped at or after the last pose has no successor in the buffer (undefined in the reference, which only
 * de-skews once a later measurement has arrived, :185-201): it gets the last pose and is counted in n_clamped. */
typedef struct {
  double time;
  double pos[3];
  double rot[4]; /* x y z w */
} so_icp_stamped_pose;
typedef struct {
  double q_w_original_l[4]; /* x y z w: orientation of the sweep-start sensor frame (featureExtraction.cpp:289) */
  double t_w_original_l[3]; /* :290 */
  uint32_t n_clamped, reserved;
} so_icp_deskew_info;
int so_icp_deskew_scan(so_icp_ctx *ctx, void *points /* host, rewritten in place */, size_t n, size_t stride_bytes,
                       size_t time_offset_bytes, double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses,
                       int poses_are_imu, const double T_i_l[7] /* tx ty tz qx qy qz qw; NULL = identity */, so_icp_deskew_info *info);
/* same on records already resident in HBM (rewritten there) */
int so_icp_deskew_scan_dev(so_icp_ctx *ctx, void *d_points, size_t n, size_t stride_bytes, size_t time_offset_bytes,
                           double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                           const double T_i_l[7], so_icp_deskew_info *info);

/* -------- the front end of featureExtraction (src/FeatureExtraction/featureExtraction.cpp) on the device: one pass from the
 * driver's sensor_msgs::PointCloud2 payload to the two clouds of a LaserFeature, in the reference's order.
 *  1. ingest (laserCloudHandler, :710-766): n = width * height points, row-major, rows row_step bytes apart, points point_step
 *     bytes apart (pcl::fromROSMsg).  Velodyne: float x y z intensity time and uint16 ring as they are.  Ouster: rot * (x, y, z)
 *     + pos of T_ouster_sensor in fp64 rounded to float (utils::transformOusterPoints), intensity, time = (float)t * 1e-9f from
 *     the uint32 t in ns, ring 0.  A field the caller found absent (offset -1; PCL matches name, datatype and count) reads 0.
 *  2. de-skew (removePointDistortion, :223-314) when n_poses > 0, exactly so_icp_deskew_scan on the ingested records;
 *     n_poses == 0 is the reference's "no IMU" branch (no de-skew).
 *  3. uniform surf sampling (uniformFeatureExtraction, :504-525): candidates i = 1, 1 + s, ... < n (s = filter_point_size),
 *     each against record i - 1, kept when |dx| > 1e-7 || |dy| > 1e-7 || (|dz| > 1e-7 && x*x + y*y + z*z > min_range^2).
 * Outputs, 32-byte records each: cloud_nodistortion as point_os::PointcloudXYZITR (x y z at 0 4 8, 0 at 12, intensity 16,
 * time 20, uint16 ring 24, zero padding), cloud_surface as pcl::PointXYZI (x y z, 1.0f at 12, intensity = the point's time at
 * 16, zero padding) in ascending i.  Little-endian payloads only. */
#define SO_ICP_SENSOR_VELODYNE 0 /* SensorType::VELODYNE */
#define SO_ICP_SENSOR_OUSTER 1   /* SensorType::OUSTER */
typedef struct {
  int32_t sensor;       /* SO_ICP_SENSOR_* */
  int32_t is_bigendian; /* PointCloud2::is_bigendian: 1 is refused */
  uint32_t point_step, row_step;
  /* byte offsets inside a point; -1 = absent or not matching (x y z intensity FLOAT32 count 1; time FLOAT32 (velodyne) or t
   * UINT32 (ouster); ring UINT16 (velodyne)) */
  int32_t off_x, off_y, off_z, off_intensity, off_time, off_ring;
  int32_t filter_point_size; /* feature_extraction_node.filter_point_size, >= 1 */
  float min_range;           /* feature_extraction_node.min_range */
  double T_ouster_sensor[7]; /* tx ty tz qx qy qz qw (parameter.cpp:270-277: R = diag(-1, -1, 1), t = (0, 0, 0.036180)) */
} so_icp_sweep_layout;
typedef struct {
  double q_w_original_l[4]; /* x y z w: so_icp_deskew_info's; identity without de-skew */
  double t_w_original_l[3]; /* zero without de-skew (the node then publishes its member from the sweep before) */
  uint32_t n_clamped;       /* so_icp_deskew_info's */
  int32_t deskewed;         /* 1: n_poses > 0 */
  uint64_t n_points;        /* width * height: records of cloud_nodistortion */
  uint64_t n_surface;       /* records of cloud_surface */
} so_icp_feature_info;
/* raw: host payload (row_step * height bytes).  nodistortion_out (n_points * 32 bytes) and surface_out (room for
 * n_points > 1 ? (n_points - 2) / filter_point_size + 1 : 0 records; n_points records always suffice) are host buffers, each
 * optional.  One copy of the payload in, one enqueue, one read-back of the counts, then the outputs. */
int so_icp_extract_features(so_icp_ctx *ctx, const void *raw, uint32_t width, uint32_t height, const so_icp_sweep_layout *layout,
                            double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                            const double T_i_l[7], void *nodistortion_out, void *surface_out, so_icp_feature_info *info);
/* same, payload already in HBM; *d_nodistortion_out and *d_surface_out (nullable) are device buffers owned by the context, valid
 * until its next so_icp_extract_features(_dev) call.  The call returns when both are complete. */
int so_icp_extract_features_dev(so_icp_ctx *ctx, const void *d_raw, uint32_t width, uint32_t height, const so_icp_sweep_layout *layout,
                                double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                                const double T_i_l[7], void **d_nodistortion_out, void **d_surface_out, so_icp_feature_info *info);
/* -------- the same front end for the Livox sensors: featureExtraction::livoxHandler
 * (src/FeatureExtraction/featureExtraction.cpp:775-823) in place of laserCloudHandler, then the same removePointDistortion
 * (:223-314) and uniformFeatureExtraction (:504-525) as above.  raw: the `points` of a livox_ros_driver2/msg/CustomMsg,
 * n_points records point_step bytes apart (the last one may end with its last field).  Per point i (:794-806):
 *   accepted iff line < n_scans && ((tag & 0x30) == 0x10 || (tag & 0x30) == 0x00); a rejected point keeps the value-initialised
 *   record of points.resize(point_num): 32 zero bytes -- which the de-skew and the sampler then treat like any other point;
 *   x y z = R_imu_laser_gravity * Vector3d(x, y, z) in fp64, each row (R[r][0]*x + R[r][1]*y) + R[r][2]*z unfused, rounded to
 *   float (always multiplied, the identity too: an infinite x makes y and z NaN, as Eigen's product does);
 *   intensity = (float)reflectivity; time = (float)offset_time / 1e9f (a correctly rounded division, :803 -- not the Ouster's
 *   multiplication by 1e-9f); ring = line.
 * R_imu_laser_gravity is imu_Init->imu_laser_R_Gravity, or the identity while the node's IMU buffer is empty (:788-791): the
 * caller's, as this library does not build imuInit.  provide_point_time: 0 (:807-810, the node shuts down) has no counterpart.
 * The offsets are data: so_icp_livox_default_layout gives those of livox_ros_driver2's CustomPoint (uint32 offset_time; float32
 * x, y, z; uint8 reflectivity, tag, line: 0 / 4 8 12 / 16 17 18, point_step 20 -- as CDR lays the sequence out and as a C++
 * std::vector<CustomPoint> does); that message definition is not part of the reference tree (unpinned). */
typedef struct {
  uint32_t point_step;
  /* byte offsets inside a point, all >= 0: offset_time UINT32 (ns from the message's timebase), x y z FLOAT32, the rest UINT8 */
  int32_t off_offset_time, off_x, off_y, off_z, off_reflectivity, off_tag, off_line;
  int32_t n_scans;           /* feature_extraction_node.scan_line (N_SCANS, default 4); 0 .. 256 */
  int32_t filter_point_size; /* feature_extraction_node.filter_point_size, >= 1 */
  float min_range;           /* feature_extraction_node.min_range */
  int32_t reserved;
  double R_imu_laser_gravity[9]; /* row-major */
} so_icp_livox_layout;
/* CustomPoint's offsets, the node's parameter defaults (:120-130: scan_line 4, filter_point_size 3, min_range 0.2), R = identity */
void so_icp_livox_default_layout(so_icp_livox_layout *layout);
/* livoxHandler (:775-823) + removePointDistortion + uniformFeatureExtraction; arguments and outputs as so_icp_extract_features.
 * raw: host, (n_points - 1) * point_step + the end of the last field bytes are read. */
int so_icp_extract_features_livox(so_icp_ctx *ctx, const void *raw, uint32_t n_points, const so_icp_livox_layout *layout,
                                  double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                                  const double T_i_l[7], void *nodistortion_out, void *surface_out, so_icp_feature_info *info);
/* same (livoxHandler, :775-823), payload already in HBM at any byte alignment; outputs as so_icp_extract_features_dev: device
 * buffers owned by the context, shared with that entry, valid until the next call of either. */
int so_icp_extract_features_livox_dev(so_icp_ctx *ctx, const void *d_raw, uint32_t n_points, const so_icp_livox_layout *layout,
                                      double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                                      const double T_i_l[7], void **d_nodistortion_out, void **d_surface_out, so_icp_feature_info *info);
/* -------- the same front end for a sweep WITHOUT per-point time (feature_extraction_node.provide_point_time: 0; older
 * velodyne_pointcloud drivers, most recorded VLP-16 / HDL-32 / HDL-64 bags): featureExtraction::assignTimeforPointCloud
 * (src/FeatureExtraction/featureExtraction.cpp:646-708, called from laserCloudHandler :753-759) in place of step 1, then the same
 * removePointDistortion and uniformFeatureExtraction on the records it leaves.  pcl::fromROSMsg into pcl::PointXYZI: float
 * x y z intensity, an absent field reads 0; the sensor type is not looked at.  Per point i of the n = width * height (:655-704):
 *   angle = atan(z / sqrt(x*x + y*y)) * 180 / M_PI as a float: the sum (unfused), sqrt and the quotient in float, atan as float
 *   (taken as the correctly rounded value), * 180 a float product, / M_PI in double, rounded to float;
 *   n_scans 16: ring = int((angle + 15) / 2 + 0.5), sum and quotient in float, + 0.5 in double; dropped when > 15 or < 0
 *           32: ring = int((angle + 92.0/3.0) * 3.0 / 4.0) in double; dropped when > 31 or < 0
 *           64: ring = angle >= -8.83 ? int((2 - angle) * 3.0 + 0.5) : 32 + int((-8.83 - angle) * 2.0 + 0.5), 2 - angle in float, the
 *               rest in double; dropped when angle > 2 || angle < -24.33 || ring > 50 || ring < 0
 *           4, 128: ring 0, nothing dropped (the "wrong scan number" branch)
 *   int() truncates toward zero (an angle of -17 degrees is ring 0 of 16).  NaN rule: a NaN angle -- (0, 0, 0), inf / inf, a NaN
 *   coordinate -- makes int(NaN), undefined in C++; it is pinned to x86-64's INT_MIN, so the point is dropped in the three tables.
 *   time = (float)(rel * scanPeriod), rel = (float)((columnTime * int(i / n_scans) + laserTime * (i % n_scans)) / scanPeriod) in
 *   double, with featureExtraction.h:91-93's constants; i is the index in the incoming sweep.
 * Loop-bound rule: a dropped point does cloud_size--; continue, and cloud_size is the loop's bound, so every drop also cuts one
 * point off the END of the sweep.  With D(i) = the number of dropped points among [0, i): index i is visited iff i + D(i) < n
 * (a prefix, as i + D(i) increases strictly); a point becomes a record iff it is visited and not dropped, at position i - D(i).
 * info->n_points is the number of these records (not width * height); de-skew and sampling see only them.
 * width * height == 0, or no record left: SO_ICP_OK, zero counts, no de-skew (deskewed 0, the identity; the reference's back() on
 * the empty cloud is undefined). */
typedef struct {
  int32_t is_bigendian; /* PointCloud2::is_bigendian: 1 is refused */
  uint32_t point_step, row_step;
  int32_t off_x, off_y, off_z, off_intensity; /* byte offsets inside a point, FLOAT32 count 1; -1 = absent or not matching */
  int32_t n_scans;                            /* feature_extraction_node.scan_line (N_SCANS): 4, 16, 32, 64 or 128 (:62); any other value is refused */
  int32_t filter_point_size;                  /* feature_extraction_node.filter_point_size, >= 1 */
  float min_range;                            /* feature_extraction_node.min_range */
} so_icp_untimed_layout;
/* assignTimeforPointCloud (:646-708) + removePointDistortion + uniformFeatureExtraction; arguments, buffer ownership and validity as
 * so_icp_extract_features, the host output buffers sized for width * height records.  The record count is known only on the
 * device, and the sampler's launch takes it as an argument: it is read back between the two launches, one synchronisation more
 * than so_icp_extract_features. */
int so_icp_extract_features_untimed(so_icp_ctx *ctx, const void *raw, uint32_t width, uint32_t height, const so_icp_untimed_layout *layout,
                                    double lidar_start_time, const so_icp_stamped_pose *poses, size_t n_poses, int poses_are_imu,
                                    const double T_i_l[7], void *nodistortion_out, void *surface_out, so_icp_feature_info *info);
/* same (assignTimeforPointCloud, :646-708), payload already in HBM; outputs as so_icp_extract_features_dev: device buffers owned by
 * the context, shared with that entry and the Livox one, valid until the next call of any of them. */
int so_icp_extract_features_untimed_dev(so_icp_ctx *ctx, const void *d_raw, uint32_t width, uint32_t height,
                                        const so_icp_untimed_layout *layout, double lidar_start_time, const so_icp_stamped_pose *poses,
                                        size_t n_poses, int poses_are_imu, const double T_i_l[7], void **d_nodistortion_out,
                                        void **d_surface_out, so_icp_feature_info *info);
/* so_icp_prefilter_scan on a cloud already in HBM and complete (e.g. *d_surface_out above, stride 32): same results, bit for bit */
int so_icp_prefilter_scan_dev(so_icp_ctx *ctx, const void *d_surf, size_t n, size_t stride_bytes, int auto_voxel_size, float line_res,
                              float plane_res, void **d_filtered_out, size_t *n_out, so_icp_prefilter_info *info);

/* The intensities of the last so_icp_prefilter_scan(_dev) output, index for index with its *d_filtered_out (per leaf: the rules at
 * so_icp_set_cloud_intensity; "leaf size too small": passed through in input order).  out: host copy of cap floats, or NULL;
 * *d_out (d_out may be NULL): device array owned by the context, valid as long as that *d_filtered_out.  The switch was off during
 * that pre-filter: *n_out = 0, SO_ICP_OK. */
int so_icp_prefilter_intensity(so_icp_ctx *ctx, float *out, size_t cap, void **d_out, size_t *n_out);

/* -------- one step after Seam A: the registered scan laserMapping::publishTopic builds
 * (src/LaserMapping/laserMapping.cpp:464-493 with utils::pointAssociateToMap, src/utils/superodom_utils.cpp:148-158).
 * Records with float x y z at byte 0 4 8, rewritten in place: a point within 0.1 m of the sensor (x*x + y*y + z*z < 0.01 in
 * float) stays as it is, every other point becomes q * p + t (fp64, rounded to float).  keep[i] (nullable) = 1 when the
 * result lies farther than 0.1 m from the world origin -- the node publishes only those; *n_kept (nullable) = their number. */
int so_icp_transform_cloud(so_icp_ctx *ctx, void *points /* host, rewritten in place */, size_t n, size_t stride_bytes,
                           const double T_w_lidar[7], uint8_t *keep, size_t *n_kept);
/* The same registered scan (laserMapping.cpp:464-493, utils::pointAssociateToMap, superodom_utils.cpp:148-158) as the node
 * publishes it, from records already in HBM and complete (e.g. *d_nodistortion_out of so_icp_extract_features(_livox)_dev, stride
 * 32): n records stride_bytes apart (>= 12, a multiple of 4; d_records 4-byte aligned; 16-byte aligned records with a stride that
 * is a multiple of 16 take the wide loads), float x y z at byte 0 4 8, not modified.  The arithmetic is so_icp_transform_cloud's;
 * a record whose result lies farther than 0.1 m from the world origin is kept: all its stride_bytes bytes with the three floats
 * replaced, in the order of the input, packed at the same stride -- so_icp_transform_cloud followed by the caller's squeeze, bit
 * for bit.  A NaN coordinate drops the record.  One launch, one copy, one synchronisation, on the auxiliary queue.
 * out (host, nullable) has room for n records: n * stride_bytes bytes are copied, the bytes behind the first *n_kept records are
 * unspecified.  *d_out (nullable) = a device buffer owned by the context with the same bytes, valid until the next
 * so_icp_registered_scan(_dev) call; no other entry writes it, and this entry writes no other entry's buffers.
 * n == 0: SO_ICP_OK, *n_kept = 0, *d_out = NULL.  SO_ICP_E_UNSUPPORTED for n >= 2^31. */
int so_icp_registered_scan_dev(so_icp_ctx *ctx, const void *d_records, size_t n, size_t stride_bytes, const double T_w_lidar[7],
                               void *out, void **d_out, size_t *n_kept);
/* same from host records (any address; not modified unless out == records, which is allowed: the squeeze in place) */
int so_icp_registered_scan(so_icp_ctx *ctx, const void *records, size_t n, size_t stride_bytes, const double T_w_lidar[7],
                           void *out, size_t *n_kept);

/* -------- multi-GPU: one process per GPU; the map is sharded by brick-hash of the voxel grid and the 45 fp64 sums of every
 * evaluation are summed over the ranks: by RCCL (below), by an in-process group, or by the solve launches themselves
 * (peer exchange, further below) -------------------------------------------------------------------------------------- */
#define SO_ICP_UNIQUE_ID_BYTES 128
int so_icp_comm_unique_id(uint8_t id[SO_ICP_UNIQUE_ID_BYTES]);                 /* rank 0: ncclGetUniqueId */
int so_icp_comm_init(so_icp_ctx *ctx, const uint8_t id[SO_ICP_UNIQUE_ID_BYTES]); /* all ranks: ncclCommInitRank on ctx->rank/world_size */
/* The same exchange without RCCL, for the shard contexts of ONE process (one thread + one context per GPU of the node, or
 * several shard contexts on one GPU in a test): the contexts that pass the same key form a group of cfg.world_size members
 * and sum their records through host memory in rank order.  Every member must run the same registrations, each from its
 * own thread (a member waits inside so_icp_register until all members have contributed).  The streams of one process share its
 * hardware queues (HIP: GPU_MAX_HW_QUEUES, 4 by default): with the peer exchange enabled, where every member's solve launch
 * must be running at the same time, keep the number of members per DEVICE at or below that. */
int so_icp_comm_init_inprocess(so_icp_ctx *ctx, uint64_t group_key);
/* Peer exchange: the per-evaluation collective replaced by the ranks' persistent solve launches trading their 45-double
 * records themselves -- tagged 16-byte chunks pushed into every rank's inbox (device memory mapped across processes with
 * hipIpc, across the contexts of one process by pointer) with system-scope stores over xGMI, polled by the receiving
 * launch.  One launch per outer iteration survives N > 1 (with a collective per evaluation the solve falls apart into
 * ~25 launches + collectives per registration).  Transport-agnostic like the unique id above:
 *   1. every rank: so_icp_peer_export -> handle;  2. exchange the handles (rank order) by any means;
 *   3. every rank, at about the same time: so_icp_peer_connect (maps the inboxes and runs a self-test with the very
 *      stores / loads of the exchange; *self_test_ok = 0 when a mapping or a chunk is missing: not an error);
 *   4. agree on the minimum of the self-test results and call so_icp_peer_enable(agreed) on every rank -- with 0 the
 *      context keeps the collective path (RCCL / in-process group).  The map-count collective of a map insert still needs
 *      one of those.  While enabled, a registration that loses a rank returns SO_ICP_E_HIP (no silent fall-back: the
 *      decision to leave the peer path would have to be collective). */
#define SO_ICP_PEER_HANDLE_BYTES 80
int so_icp_peer_export(so_icp_ctx *ctx, uint8_t handle[SO_ICP_PEER_HANDLE_BYTES]);
int so_icp_peer_connect(so_icp_ctx *ctx, const uint8_t *handles /* world_size x SO_ICP_PEER_HANDLE_BYTES, rank order */, int *self_test_ok);
int so_icp_peer_enable(so_icp_ctx *ctx, int on);
/* brick-hash ownership of the shard (host logic, testable without a GPU) */
int so_icp_shard_owner_of_point(const float p[3], const int origin[3], float plane_res, int world_size);
int so_icp_cells_per_cube(float plane_res, double *cell_size);
/* how a scan's queries fall to the ranks under `pose` (the ownership rule of the sharded registration; host arithmetic):
 * counts[r] = queries whose map cell rank r owns (queries outside the window count for rank 0, like in the kernels) */
int so_icp_shard_histogram(const float *scan_xyz, size_t n, size_t stride_bytes, const double pose[7], const int origin[3],
                           float plane_res, int world_size, int64_t *counts /* world_size */);

/* -------- host-side Levenberg-Marquardt state machine (the Ceres restatement the device path is
 * driven by; exposed so it can be tested without a GPU) ------------------------------------------ */
typedef struct {
  double cost;      /* 0.5 * sum c_i rho(s_i) */
  double count;     /* accepted correspondences */
  double Jtr[6];
  double JtJ[21];   /* upper triangle, row-major: (0,0..5),(1,1..5),... */
  double hist[16];  /* reject_hist[7] then obs_hist[9] (carried through the same all-reduce) */
} so_icp_sums;      /* 45 doubles */
typedef struct { double opaque[96]; } so_icp_lm_state;
/* begin: sums evaluated at x0. returns 1 and writes next_pose when another evaluation is needed, 0 when done */
int so_icp_lm_begin(so_icp_lm_state *s, const double x0[7], const so_icp_sums *sums_at_x0, int max_iterations, double next_pose[7]);
int so_icp_lm_feed(so_icp_lm_state *s, const so_icp_sums *sums_at_next, double next_pose[7]);
int so_icp_lm_result(const so_icp_lm_state *s, double pose[7], so_icp_iter_stats *stats /* solver fields only */);

/* -------- SEAM C: for a caller that keeps its own solver.  The reference rebuilds its Ceres problem on every outer ICP iteration
 * from extractFeaturesConstraints (LS.cpp:119-133, 299-344); a host that adds factors of its own to that problem (the absolute pose
 * prior of addAbsolutePoseConstraints, an iterated-EKF front end that needs n, d, p per iteration) cannot use Seam A, which solves.
 * so_icp_match is one pass of extractFeaturesConstraints at a pose of the caller's; so_icp_correspondence_sums is the evaluation of
 * the set it left at the poses the caller's solver tries.  The loop  match -> host solve (sums per candidate) -> match ...  with
 * so_icp_lm_begin / so_icp_lm_feed as the solver is so_icp_register (tests/seam_c_ref.py register_through_seam).
 *
 * so_icp_match / so_icp_match_dev: the matching half of one outer iteration at `pose` -- sub-sampling, world transform, 5-NN, plane fit
 * and gates, residualCoefficient, both histograms -- and the evaluation at `pose`: what a registration from `pose` does before its
 * first LM step, through the registration's own kernels (one outer iteration, no LM iteration, one launch per evaluation).
 * stats: n_iterations = 1; iterations[0] holds num_surf_from_scan, reject_hist, obs_hist and initial_cost == final_cost, with
 * lm_iterations = num_successful_steps = termination = 0 and pose_after = pose (termination is so_icp_lm_begin's for max_iterations 0:
 * 4 when no point was accepted, 3 when the gradient at `pose` is already below tolerance); JtJ / Jtr are at `pose`.  Return codes are
 * so_icp_register's (SO_ICP_NOT_ENOUGH_MAP_FEATURES included); the map window is placed as so_icp_register places it for `pose`.
 * Needs so_icp_keep_correspondences(ctx, 1) (SO_ICP_E_INVALID otherwise): the match leaves its set as "the last registration's" --
 * outer_iteration 0, pose_fit = pose_eval = pose -- for so_icp_correspondences and so_icp_correspondence_sums.
 * Left alone: the previous observability histogram (so_icp_stats::uncertainty of later calls), startup_count, the tracker's last pose
 * and time, the map's contents, scans announced with so_icp_stage_scan / so_icp_sequence_announce_next (a staged copy of this very
 * buffer is not consumed: the match uploads it again), the chain of so_icp_register_sequence, so_icp_timing::registrations.
 * world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP. */
int so_icp_match(so_icp_ctx *ctx, const float *scan_xyz, size_t n, size_t stride_bytes, const double pose[7], so_icp_stats *stats);
int so_icp_match_dev(so_icp_ctx *ctx, const void *d_scan_xyz, size_t n, const double pose[7], so_icp_stats *stats);
/* Cost and loss-corrected normal equations of the KEPT set (whichever call left it: a registration entry or so_icp_match) at n_poses
 * poses, summed on the device: per pose cost, count (= n_accepted), Jtr[6], JtJ[21] (upper triangle) with
 * J = [n, p x (R^T n)], JtJ += weight J J^T, Jtr += weight residual J, residual and weight as in so_icp_correspondence, with the a^2
 * and Tukey variant of the call that formed the set; hist[16] = the reject and observability histograms of the outer iteration that
 * formed it (constant over the poses: what so_icp_lm_begin / _feed carry through).  sums_out[k] is what so_icp_lm_begin / so_icp_lm_feed take.
 * Every sum is a fixed tree (a thread's points in order, a butterfly over the wavefront, the four wavefronts in order, the 1 024-point
 * tiles in tile order; no atomics): two calls give the same bits, pose k's sums do not depend on the other poses of the call, and cost
 * is so_icp_correspondences(pose).cost bit for bit.  The points are read once per call, whatever n_poses; two launches, one copy of
 * the poses in, one of n_poses x 45 doubles out, one synchronisation, on the context's queue.
 * Nothing kept (the switch off, no set, info.valid would be 0): SO_ICP_OK and every output zero.  NULL poses / sums_out or n_poses
 * outside 1 .. SO_ICP_SUMS_MAX_POSES: SO_ICP_E_INVALID.  A host-only context: SO_ICP_E_HIP. */
#define SO_ICP_SUMS_MAX_POSES 64
int so_icp_correspondence_sums(so_icp_ctx *ctx, const double *poses /* n_poses x 7 */, int n_poses, so_icp_sums *sums_out /* n_poses */);

/* -------- ABSOLUTE POSE PRIOR inside the device solve.  The reference's Ceres problem holds, beside the point-to-plane factors, one
 * SE3AbsolutatePoseFactor (addAbsolutePoseConstraints, LS.cpp:285-297; SE3AbsolutatePoseFactor.cpp:9-51): in a degenerate scene the VIO
 * pose holds the axes the lidar cannot observe.  It is one 6-row residual block, so it adds nothing per point: added to the 29 sums of
 * every evaluation it is the same Ceres problem, and the registration stays one enqueue on the device.  At a pose {t, q = x y z w}
 *   e[0..2] = t - t_m,  qe = conj(q_m) (x) q,  e[3..5] = 2 vec(qe)                       (qe as it is, factor :21-26)
 *   B = blockdiag(I3, w' I3 + [v']x), (v', w') = qe negated when qe.w < 0               (in the Jacobian only, factor :41-43)
 *   d_i = sqrt(max(count_floor[i], trunc(count * count_fraction[i]))) where count_floor[i] > 0, else 1;  count = the sums' count word
 *   r = D U e,  J = D U B;   cost += r'r / 2,  Jtr += J'r,  JtJ += J'J;   count and hist stay.
 * count_floor / count_fraction state the reference's information exactly (std::max(50, int(good_feature_num * 0.1)), LS.cpp:289-294).
 * T_meas' quaternion is used as given (a unit quaternion is the caller's business).  The sign rule of B is Utility::Qleft's positify as its name
 * states it (in the reference checkout this was written against its sign flip is commented out, utility.h:37-44): where qe.w < 0 -- T_meas given with the other sign, or more than 180 degrees away -- J is MINUS the derivative of r. */
typedef struct {
  double T_meas[7];             /* T_w_i_meas_ */
  double sqrt_information[36];  /* row-major U, residual = U e: what SE3AbsolutatePoseFactor.h:20-23 keeps (L^T of the LLT) */
  double count_floor[6], count_fraction[6];   /* all zero: U as given */
} so_icp_pose_prior;            /* 55 doubles */
/* U = L^T of the host LLT of `information` (row-major, its lower triangle is read), T_meas copied, count_floor / count_fraction zero.
 * SO_ICP_E_INVALID when the matrix is not positive semi-definite with a non-negative diagonal; a zero pivot with a zero column below
 * it is allowed (the reference's information(5,5) is 0) and gives a zero row. */
int so_icp_pose_prior_from_information(const double information[36], const double T_meas[7], so_icp_pose_prior *out);
/* Host only, no context: adds the prior at `pose` to *inout as above (one fp64 addition per word, the sum that was there on the left),
 * reading inout->count for the row scale.  Bit for bit what the device adds: a Seam C host loop with this call behind every
 * so_icp_correspondence_sums is the registration with the prior set. */
int so_icp_pose_prior_sums(const so_icp_pose_prior *prior, const double pose[7], so_icp_sums *inout);
/* ONE-SHOT: the prior goes into the next call of so_icp_register, so_icp_register_dev, so_icp_localization or so_icp_localization_dev
 * (scan staged or not) and is consumed when that call returns, whatever it returns -- also a localization frame that seeds the map
 * (initialization = 0) and a call that finds too little map.  A registration the context repeats by itself (SO_ICP_FLAG_RETRIED) keeps
 * it for the repeat.  In that registration every evaluation the controller sees carries the prior; initial_cost, final_cost,
 * so_icp_stats::JtJ and Jtr include it (the normal equations of the Ceres problem, as ceres::Covariance would see them);
 * prediction_source = 1 (LS.cpp:297) and SO_ICP_FLAG_POSE_PRIOR is set.  num_surf_from_scan stays the number of plane correspondences,
 * and an evaluation with none still ends the solve with termination 4 -- Ceres would solve the prior alone there, the reference returns
 * before it gets that far (LS.cpp:113-116).  so_icp_correspondences and so_icp_correspondence_sums keep reporting the planes only.
 * While a prior is pending so_icp_register_batch, so_icp_register_sequence, so_icp_localization_sequence, so_icp_match(_dev) and
 * so_icp_set_batch_priors return SO_ICP_E_UNSUPPORTED and leave it pending; this call is refused while the priors of a run or of a
 * batch are pending.  prior == NULL withdraws a pending prior.
 * world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP; a non-finite field or a T_meas quaternion of zero norm:
 * SO_ICP_E_INVALID.  Setting is host work only (the prior travels as an argument of that registration's solve launches); a context on
 * which no prior was ever set does nothing more than before in any entry. */
int so_icp_set_pose_prior(so_icp_ctx *ctx, const so_icp_pose_prior *prior /* NULL withdraws */);

/* One prior PER FRAME of a run: ONE-SHOT, for the next so_icp_register_sequence or so_icp_localization_sequence call, which stays
 * chained.  modes[k] says where frame k's measurement comes from:
 *   NONE      frame k carries no prior: bit for bit and flag for flag the frame of a run without priors
 *   GIVEN     priors[k] as it stands
 *   AT_GUESS  priors[k] with T_meas replaced by the frame's own guess (guesses_out[k]); priors[k].T_meas is not read.  The reference
 *             puts its prior on `position`, the frame's initial guess (LS.cpp:131, 224-226, 295); in a chained run the host never sees
 *             the guess of frame k >= 1 before it enqueues that frame -- the solve that ends frame k - 1 forms it on the device --, so
 *             "hold the unobservable axes at the prediction" is stated here and the measurement taken where the guess is formed.
 * With P_k = priors[k] (AT_GUESS: T_meas := guesses_out[k]), frame k of so_icp_register_sequence is bit for bit
 * so_icp_set_pose_prior(ctx, P_k) + so_icp_register from guesses_out[k], and frame k of so_icp_localization_sequence that call +
 * so_icp_localization(initialization = 1), the map after every frame included -- chained or not, and across a broken chain.  A frame
 * with a prior reports like the single entry: costs, JtJ and Jtr include it, prediction_source = 1, SO_ICP_FLAG_POSE_PRIOR.
 * Both arrays are copied.  The next sequence call consumes the priors when it returns, whatever it returns; a call whose `count`
 * differs returns SO_ICP_E_INVALID before it touches anything and leaves them pending.  count == 0 or priors == NULL withdraws.
 * While the priors of a run are pending so_icp_register(_dev), so_icp_localization(_dev), so_icp_register_batch, so_icp_match(_dev),
 * so_icp_set_pose_prior and so_icp_set_batch_priors return SO_ICP_E_UNSUPPORTED and leave them pending; a pending single prior is
 * refused by both sequence entries as before, and by this call, and so are the pending priors of a batch.  Validation as so_icp_set_pose_prior's, on the words a mode reads: a non-finite field or (GIVEN)
 * a T_meas quaternion of zero norm SO_ICP_E_INVALID, a mode above 2 SO_ICP_E_INVALID, world_size > 1 SO_ICP_E_UNSUPPORTED, a host-only
 * context SO_ICP_E_HIP.  Not in a run: the reference's uncertainty-scaled information (frame k's U would need frame k - 1's
 * uncertainty, which the host does not have when it enqueues a chained frame). */
#define SO_ICP_PRIOR_NONE     0
#define SO_ICP_PRIOR_GIVEN    1
#define SO_ICP_PRIOR_AT_GUESS 2
int so_icp_set_sequence_priors(so_icp_ctx *ctx, int count, const so_icp_pose_prior *priors /* count */,
                               const uint8_t *modes /* count; NULL = all GIVEN */);

/* One prior PER HYPOTHESIS of a batch: ONE-SHOT, for the next so_icp_register_batch call, inside its batched solve launches.  modes[h]:
 *   NONE      hypothesis h carries no prior: bit for bit and flag for flag the hypothesis of a batch without priors
 *   GIVEN     priors[h] as it stands
 *   AT_GUESS  priors[h] with T_meas replaced by poses_in[h] of that batch call; priors[h].T_meas is not read
 * With P_h = priors[h] (AT_GUESS: T_meas := poses_in[h]), hypothesis h of the batch is bit for bit so_icp_set_pose_prior(ctx, P_h) +
 * so_icp_register from poses_in[h] on a context with the same map and history (`uncertainty` is carried over from the call before, as
 * in every batch) -- on every path a batch can take: groups of more than 64, one workgroup per compute unit, chained rounds or not, a
 * repeated group, concurrent registrations on worker contexts (SOICP_BATCH_MODE=lanes, an empty scan).  A hypothesis with a prior
 * reports like the single entry: costs, JtJ and Jtr include it, prediction_source = 1, SO_ICP_FLAG_POSE_PRIOR; num_surf_from_scan counts
 * the planes, and a pass with none ends with termination 4.  A batch whose priors are all NONE launches what a batch without launches.
 * Both arrays are copied.  The next so_icp_register_batch takes the priors out of the context when it starts: they are gone when it
 * returns, whatever it returns (too little map -- then no flag is set --, an error); a call whose n_hyp differs (n_hyp == 0 too)
 * returns SO_ICP_E_INVALID before it touches anything and leaves them pending.  n_hyp == 0 or priors == NULL withdraws.
 * While the priors of a batch are pending so_icp_register(_dev), so_icp_localization(_dev), so_icp_register_sequence,
 * so_icp_localization_sequence, so_icp_match(_dev), so_icp_set_pose_prior and so_icp_set_sequence_priors return SO_ICP_E_UNSUPPORTED
 * and leave them pending; this call is refused while a single prior or the priors of a run are pending.  Validation as
 * so_icp_set_sequence_priors'.  Not in a batch: the reference's uncertainty-scaled information (the caller scales U). */
int so_icp_set_batch_priors(so_icp_ctx *ctx, int n_hyp, const so_icp_pose_prior *priors /* n_hyp */,
                            const uint8_t *modes /* n_hyp; NULL = all GIVEN */);

/* -------- the correspondence sets of a BATCH's hypotheses: which points each hypothesis matched, how the cost of its set behaves around
 * its result, whether two hypotheses that ended at different poses explain the same points -- without registering them one by one.
 * The switch.  A new context has it off, and while it is off so_icp_register_batch enqueues, allocates, copies and synchronises exactly
 * what it does without this feature, and both exports below report valid = 0 / zero sums.  While it is on, a batch leaves in memory the
 * context owns and no other entry writes: the plane, coefficient and status arrays of ALL n_hyp hypotheses (41 bytes per point and
 * hypothesis; the batched kernels write them there instead of into the batch's working arrays -- other kernel arguments, the same
 * kernels -- and the concurrent registrations of SOICP_BATCH_MODE=lanes, of an empty scan or of a degraded context each copy theirs
 * there on their own queue), ONE packed copy of the scan (12 n bytes, device to device, in front of the batch's first launch) and per
 * hypothesis what a single registration keeps: the accepted count, the loss, outer_iteration, pose_fit, pose_eval, both histograms,
 * and valid = (rc_out[h] == SO_ICP_OK).  The set is replaced by the next so_icp_register_batch or so_icp_match_batch (which leaves none if it
 * fails); nothing else invalidates it: not a single registration, a single match, a map insert, a pre-filter or so_icp_set_resolution.  Turning the switch
 * off drops the set and frees its memory.  Independent of so_icp_keep_correspondences: a batch still ends "the last registration's"
 * set.  world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP. */
int so_icp_keep_batch_correspondences(so_icp_ctx *ctx, int on);
/* so_icp_correspondences for a SELECTION of the last batch's hypotheses in one launch.  Entry k of the selection is hypothesis hyp[k]
 * (hyp == NULL: k); indices may repeat and come in any order; one outside 0 .. n_hyp - 1 of that batch: SO_ICP_E_INVALID.  n_sel is
 * 0 .. SO_ICP_BATCH_MAX_SELECTION (SO_ICP_E_INVALID beyond).  poses (nullable): entry k is evaluated at poses[7 k ..]; NULL = each
 * hypothesis' own pose_eval.  info[k] is what so_icp_correspondences reports on a context that ran hypothesis hyp[k] alone with
 * so_icp_keep_correspondences on -- counts, outer_iteration, pose_fit, pose_eval and cost, bit for bit; a hypothesis whose rc_out was not
 * SO_ICP_OK has valid = 0 and no records.  Every info[k].valid is 0 (SO_ICP_OK, nothing else touched) while the switch is off or no
 * batch has left a set.
 * Outputs, each nullable:
 *  records       the records of entry k at [first_record[k], first_record[k + 1]), ascending index, with residual and weight at the
 *                entry's pose (there is no residual_out: the records carry the residuals); NULL or cap_records < first_record[n_sel]:
 *                counts, first_record, info and cost only
 *  first_record  n_sel + 1 offsets, formed on the host from the accepted counts the hypotheses reported
 *  status_out    [k * n_points + i] = the MatchingResult byte of point i under hypothesis hyp[k] (a row of 254 for an entry with valid = 0);
 *                needs cap_status >= n_sel * n_points (SO_ICP_E_INVALID otherwise)
 *  *d_records_out  a device buffer owned by the context with the same record bytes, valid until the next so_icp_batch_correspondences
 *                call; no other entry writes it
 * One memset of the counters, one launch, one copy per requested host output and one of the counts and tile sums, one synchronisation,
 * on the context's queue.  The kernel's count of every entry is held to the reported one (SO_ICP_E_HIP with a text otherwise). */
#define SO_ICP_BATCH_MAX_SELECTION 1024
int so_icp_batch_correspondences(so_icp_ctx *ctx, const int32_t *hyp /* n_sel, NULL = 0 .. n_sel-1 */, int n_sel,
                                 const double *poses /* n_sel x 7, nullable: each hypothesis' own pose_eval */,
                                 so_icp_correspondence *records, size_t cap_records,
                                 uint64_t *first_record /* n_sel + 1 */,
                                 uint8_t *status_out /* n_sel x n_points, nullable */, size_t cap_status,
                                 void **d_records_out, so_icp_correspondence_info *info /* n_sel */);
/* so_icp_correspondence_sums for a selection (as above) of the last batch's hypotheses: sums_out[k * n_poses + j] = the sums of
 * hypothesis hyp[k]'s set at poses[(k * n_poses + j) * 7 ..], bit for bit what so_icp_correspondence_sums returns on a context that ran
 * that hypothesis alone (the same per-point expression, the same tree, the tiles added in tile order; no atomics, nothing to clear),
 * with that hypothesis' histograms.  A hypothesis without a set: zero sums.  As in the single path a hypothesis that carried a pose
 * prior (so_icp_set_batch_priors) gets the sums of its planes only: the caller adds so_icp_pose_prior_sums.  Two launches for the whole
 * selection.  n_poses outside 1 .. SO_ICP_SUMS_MAX_POSES, n_sel outside 0 .. SO_ICP_BATCH_MAX_SELECTION, an index outside the batch:
 * SO_ICP_E_INVALID. */
int so_icp_batch_correspondence_sums(so_icp_ctx *ctx, const int32_t *hyp, int n_sel,
                                     const double *poses /* n_sel x n_poses x 7 */, int n_poses /* 1 .. SO_ICP_SUMS_MAX_POSES */,
                                     so_icp_sums *sums_out /* n_sel x n_poses */);

/* -------- SEAM C for a BATCH: so_icp_match for ONE scan at n_poses poses in one call -- a caller that solves on the host (a
 * multi-hypothesis iterated EKF, a back end with factors of its own per hypothesis) or only scores poses (cost, accepted count, normal
 * equations and observability histogram over a grid of perturbations: an alignment-risk estimate) without n_poses single matches, each
 * with its own binning, sweep, evaluation and synchronisation, and without n_poses registrations whose solves it throws away.
 * Scan arguments, return value and rc_out are so_icp_register_batch's: d_scan_xyz != NULL takes a resident scan, else scan_xyz is
 * uploaded once; the call returns the number of poses that ended SO_ICP_OK, or a negative error.
 * stats[h] is, to the bit, what so_icp_match_dev reports for the same scan at poses[h] on a context of its own (same map, plane_res,
 * max_surface_features and Tukey variant): n_iterations = 1, the whole of iterations[0] (counts, both histograms, initial_cost ==
 * final_cost, pose_after = poses[h], zeros in the LM fields, so_icp_match's termination), JtJ, Jtr, pos_in_localmap and
 * laser_cloud_surf_from_map_num.  Exempt: time_elapsed_ms (the wall time of the hypothesis' group of up to 64) and flags -- the batch
 * sets SO_ICP_FLAG_HOST_MAP and SO_ICP_FLAG_COPY_READBACK where they hold, as so_icp_register_batch does, and none of the bits that
 * describe a single registration's schedule (SO_ICP_FLAG_PER_EVAL_LAUNCHES, _QUERY_WAVES, _BINNED_AHEAD, _STAGED_SCAN).
 * The map window is shifted ONCE, for poses[0], as in so_icp_register_batch: the bit-for-bit statement holds for poses that lie in the
 * map block of poses[0] (a single match at a pose of another block would have rolled the window for it).
 * The entry needs no keep switch.  With so_icp_keep_batch_correspondences on it leaves the batch's kept set -- every pose's slice, one
 * scan copy, per pose outer_iteration 0 and pose_fit = pose_eval = poses[h] -- and so_icp_batch_correspondences /
 * so_icp_batch_correspondence_sums work on it unchanged: entry h equals what so_icp_correspondences / so_icp_correspondence_sums give
 * after the single match.  With the switch off the stats are the same bytes and a set an earlier batch left is dropped.  The single
 * registration's set (so_icp_keep_correspondences) is not touched.
 * Left alone: everything so_icp_match leaves alone (the previous observability histogram, startup_count, the tracker's last pose and
 * time, the map's contents, announced and staged scans, the chain of so_icp_register_sequence, so_icp_timing::registrations), and the
 * statistics by which later so_icp_register_batch calls chain their rounds.
 * One launch fits and evaluates every (pose, point) of a group (3 binning launches, 1 sweep, that launch, one read-back); no workgroup
 * of it waits for another, so SOICP_BATCH_MODE, SOICP_BATCH_CHAIN and the fall-backs of so_icp_register_batch (one workgroup per compute
 * unit, lanes) do not apply to it: any n_poses goes through in groups of 64.
 * Refusals: a pending prior of any kind (so_icp_set_pose_prior, _sequence_priors, _batch_priors): SO_ICP_E_UNSUPPORTED, and the prior
 * stays pending; world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP; NULL poses or stats, n_poses < 0, n > 0
 * without a scan: SO_ICP_E_INVALID; n of 2^21 or more: so_icp_register_batch's refusal.  n_poses == 0 returns 0.  A 5x5x5 surf count
 * <= 50: every rc_out[h] = SO_ICP_NOT_ENOUGH_MAP_FEATURES and the call returns 0.  n == 0: every pose reports what so_icp_match
 * reports for an empty scan. */
int so_icp_match_batch(so_icp_ctx *ctx, const float *scan_xyz, const void *d_scan_xyz, size_t n, size_t stride_bytes,
                       const double *poses /* n_poses x 7 */, int n_poses,
                       so_icp_stats *stats /* n_poses */, int32_t *rc_out /* n_poses, nullable */);

/* -------- the correspondence sets of a RUN's frames: so_icp_register_sequence and so_icp_localization_sequence are the entries for a
 * backlog of feature clouds or a log replayed at full speed, and the callers of the export -- a factor-graph back end that wants
 * point-to-plane factors (the reference's features_corres, LS.h:209-222) instead of one pose per frame, colouring or masking registered
 * scans by residual -- are log-replay callers: they want the planes of EVERY frame, not of the last one.
 * The switch.  A new context has it off, and while it is off both sequence entries enqueue, allocate, copy and synchronise exactly what
 * they do without this feature, and both exports below report valid = 0 / zero sums.  While it is on, a call of either entry leaves in
 * memory the context owns and no other entry writes, per frame: the plane, coefficient and status arrays of the frame's last fit pass
 * (41 bytes per point), a packed copy of the frame's scan (12 bytes per point) -- 53 bytes per point and frame, sized by the sum of the
 * frames' points, reserved before the run's first launch (nothing is allocated under a registration in flight; when it cannot be had the
 * call returns SO_ICP_E_NOMEM before it touches anything) -- and what a single registration keeps: the accepted count, the loss of THAT
 * frame, outer_iteration, pose_fit, pose_eval, both histograms, and valid = (the frame ended with SO_ICP_OK).  Frames from the one that
 * stopped the run onwards, and every frame of a call that returned an error, have valid = 0.
 * How the records get there: a frame the chained path of so_icp_register_sequence starts itself -- chained or not -- runs the same
 * kernels with its slice of the set as their arguments (no copy, nothing between two chained registrations on the context's queue); a
 * frame that goes through a per-frame entry (SOICP_SEQ_CHAIN=0, an empty scan, a frame the chained path cannot start, every frame of
 * so_icp_localization_sequence) copies the context's three arrays into its slice behind its report, device to device on the context's
 * queue -- in front of the map insert of so_icp_localization_sequence.  The scan copies of frames started by the chained path ride on the
 * sequence's own copy queue, behind the scan's arrival or its binning, and the call waits for that queue before it returns.
 * The set is replaced by the next sequence call of either kind (which leaves none if it fails before frame 0); nothing else
 * invalidates it: not a single registration, a batch, a match, a map insert, a pre-filter or so_icp_set_resolution.  Turning the switch
 * off drops the set and frees its memory.  Independent of so_icp_keep_correspondences and so_icp_keep_batch_correspondences: with the
 * single switch on as well, the run's last frame still leaves "the last registration's" set, with the bytes it has without this switch.
 * world_size > 1: SO_ICP_E_UNSUPPORTED; a host-only context: SO_ICP_E_HIP. */
int so_icp_keep_sequence_correspondences(so_icp_ctx *ctx, int on);
/* so_icp_correspondences for a SELECTION of the last run's frames in one launch.  Entry k of the selection is frame frames[k]
 * (frames == NULL: k); indices may repeat and come in any order; one outside the kept run: SO_ICP_E_INVALID.  n_sel is
 * 0 .. SO_ICP_SEQUENCE_MAX_SELECTION (SO_ICP_E_INVALID beyond).  poses (nullable): entry k is evaluated at poses[7 k ..]; NULL = each
 * frame's own pose_eval.  info[k], the records, the status row and cost of entry k are, bit for bit, what so_icp_correspondences
 * reports on a context that registered that frame alone from guesses_out[frames[k]] (with the frame's prior, if the run had priors)
 * with so_icp_keep_correspondences on.  A frame without a set has valid = 0, no records and n_points = its points; a frame of 0 points
 * has valid = 1 and zero counts.  Every info[k] is zero (SO_ICP_OK, nothing else touched) while the switch is off or no run has left a set.
 * Outputs, each nullable:
 *  records       the records of entry k at [first_record[k], first_record[k + 1]), ascending index, with residual and weight at the
 *                entry's pose; NULL or cap_records < first_record[n_sel]: counts, offsets, info and cost only
 *  first_record  n_sel + 1 offsets, formed on the host from the accepted counts the frames reported
 *  status_out    [first_status[k] + i] = the MatchingResult byte of point i of frame frames[k] (254s for an entry with valid = 0); the
 *                frames differ in their points, so row k is info[k].n_points long; needs cap_status >= the points of all selected
 *                frames (SO_ICP_E_INVALID otherwise)
 *  first_status  n_sel + 1 offsets of the status rows
 *  *d_records_out  a device buffer owned by the context with the same record bytes, valid until the next
 *                so_icp_sequence_correspondences call; no other entry writes it
 * One memset of the counters, one launch, one copy per requested host output and one of the counts and tile sums, one synchronisation,
 * on the context's queue.  The kernel's count of every entry is held to the reported one (SO_ICP_E_HIP with a text otherwise). */
#define SO_ICP_SEQUENCE_MAX_SELECTION 1024
int so_icp_sequence_correspondences(so_icp_ctx *ctx, const int32_t *frames /* n_sel, NULL = 0 .. n_sel-1 */, int n_sel,
                                    const double *poses /* n_sel x 7, nullable: each frame's own pose_eval */,
                                    so_icp_correspondence *records, size_t cap_records, uint64_t *first_record /* n_sel + 1 */,
                                    uint8_t *status_out, size_t cap_status, uint64_t *first_status /* n_sel + 1, nullable */,
                                    void **d_records_out, so_icp_correspondence_info *info /* n_sel */);
/* so_icp_correspondence_sums for a selection (as above) of the last run's frames: sums_out[k * n_poses + j] = the sums of frame
 * frames[k]'s set at poses[(k * n_poses + j) * 7 ..], bit for bit what so_icp_correspondence_sums returns on a context that registered
 * that frame alone (the same per-point expression, the same tree, the tiles added in tile order; no atomics, nothing to clear), with
 * that frame's histograms.  A frame without a set: zero sums.  As everywhere else a frame that carried a pose prior
 * (so_icp_set_sequence_priors) gets the sums of its planes only: the caller adds so_icp_pose_prior_sums.  Two launches for the whole
 * selection.  n_poses outside 1 .. SO_ICP_SUMS_MAX_POSES, n_sel outside 0 .. SO_ICP_SEQUENCE_MAX_SELECTION, an index outside the run:
 * SO_ICP_E_INVALID. */
int so_icp_sequence_correspondence_sums(so_icp_ctx *ctx, const int32_t *frames, int n_sel,
                                        const double *poses /* n_sel x n_poses x 7 */, int n_poses /* 1 .. SO_ICP_SUMS_MAX_POSES */,
                                        so_icp_sums *sums_out /* n_sel x n_poses */);

/* -------- measurement ------------------------------------------------------------------------ */
int so_icp_get_timing(so_icp_ctx *ctx, so_icp_timing *t);
int so_icp_reset_timing(so_icp_ctx *ctx);
/* switch so_icp_config::time_kernels on a live context (e.g. 1 inside a timed region, 2 for a profiling pass after it) */
int so_icp_set_time_kernels(so_icp_ctx *ctx, int mode);
int so_icp_synchronize(so_icp_ctx *ctx);
/* test aid: MatchingResult (LS.h:85-94) of every query of the last registration's LAST outer iteration, indexed like the scan
 * (254 = not sampled / not owned by this rank) */
int so_icp_debug_match_status(so_icp_ctx *ctx, uint8_t *out, size_t n);
/* test aid: the five neighbours (canonical map indices, nearest first) the LAST k-NN sweep of the last registration left for every query, indexed
 * like the scan: out[5 * n].  Meaningful where that sweep found five neighbours inside the gate (every query the fit pass then judged: status
 * 0, 3, 4, 5); elsewhere the entries are whatever an earlier sweep left */
int so_icp_debug_neighbours(so_icp_ctx *ctx, uint32_t *out, size_t n);
/* test aid: the plane the export of so_icp_correspondence_geometry refits from its snapshot -- n[3], d, coeff (five doubles, 40 bytes)
 * per accepted point, in the records' order -- to be held to so_icp_correspondences' records bit for bit.  One launch of the export
 * kernel of its own; valid = 0 cases return SO_ICP_OK with *n_out = 0; cap < n_accepted: SO_ICP_E_INVALID */
int so_icp_debug_correspondence_refit(so_icp_ctx *ctx, double *out, size_t cap, size_t *n_out);
/* test aid: the DEVICE forms of the LM controller on a scripted sequence of sums -- no scan, no map.  The controller is a pure state
 * machine of (x0, sequence of sums), so a script drives any of its branches deterministically.
 *   form 0  the lane-parallel controller of the persistent solve (kernels.hip: lm_control_wave), run by one wavefront the way the solve's
 *           finishing workgroup runs it: sums, state and loop bounds in LDS, the hand-off record stored to global memory
 *   form 1  the one-thread controller (lm_solver.h through lm_control), by launching the production lm_step_kernel once per entry --
 *           the very kernel of the sharded path
 * Everything runs on a scratch state block owned by the call; the context's registration state is not touched.  An entry whose
 * new_solve is set is the evaluation at the solve's start (slot 0: the start is x0 for the first solve, the pose the solve before
 * ended with afterwards); the others are evaluations at the pose handed on by the entry before.  An entry is skipped, as the
 * launches of a registration skip a pass, once the registration is over or while no solve is running.
 * LIMIT: lm_control_wave is force-inlined, so form 0 is a second compilation of its source, not the instance inside the persistent
 * solve kernel: this checks the source's semantics and its equality with the one-thread form, not that kernel's machine code. */
#define SO_ICP_LM_SCRIPT_MAX 64
typedef struct {
  so_icp_sums sums;
  int32_t new_solve, reserved;
} so_icp_lm_script_entry;
typedef struct {
  int32_t more, reserved;   /* the controller's return value (0 for a skipped entry) */
  double pose[7];           /* the next pose as handed on: form 0 the pose_out copy of the hand-off, form 1 the state block's eval_pose
                               (which the one-thread form writes only when more == 1) */
  uint32_t hand[8][4];      /* form 0: the eight 16-byte hand-off chunks {value lo, value hi, tag lo, tag hi}: chunks 0..6 the pose, chunk 7
                               `more`; all ones where the entry was skipped.  form 1: zero */
  so_icp_lm_state state;    /* the controller state after the entry */
} so_icp_lm_script_step;
typedef struct {
  so_icp_lm_state state;
  double T[7], eval_pose[7], T_final[7];
  double JtJ[36], Jtr[6];
  int32_t lm_more, outer_iter, n_iterations, reg_done;
  uint32_t done_count, reserved;
  so_icp_iter_stats iterations[SO_ICP_MAX_OUTER];  /* the scratch block starts zeroed: records no solve wrote stay zero */
} so_icp_lm_script_result;
int so_icp_debug_lm_script(so_icp_ctx *ctx, int form, const double x0[7], int lm_max, int max_outer, int outer_iter,
                           const so_icp_lm_script_entry *entries, int n_entries /* 1 .. SO_ICP_LM_SCRIPT_MAX */, uint64_t want /* hand-off tag */,
                           so_icp_lm_script_step *steps /* n_entries */, so_icp_lm_script_result *result);
/* profiling aid: wall-clock stamps (100 MHz ticks) of the phases of the last fit / evaluation kernels (SOICP_ABLATE=128) */
int so_icp_debug_stamps(so_icp_ctx *ctx, uint64_t out[16]);
/* profiling aid: per-workgroup records (16 words each, 2 sweeps x workgroups) of the k-NN kernel's phases (SOICP_ABLATE=128);
 * call with out == NULL to query the size in 64-bit words */
int so_icp_debug_knn_stamps(so_icp_ctx *ctx, uint64_t *out, size_t capacity_words, size_t *n_words);

#ifdef __cplusplus
}
#endif
#endif /* SO_ICP_H */
