"""ctypes binding of libsoicp.so (include/so_icp.h).

This is the thin host-side mirror used by tests and bench.py.  The reference's host is C++
(LidarSLAM, src/LidarProcess/LidarSlam.cpp); its C++ adapter is shown in INTEGRATION.md.  Loading
fails loudly when the library is missing or when no HIP device is usable -- there is no CPU path."""
import ctypes as C
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libsoicp.so")
N_REJECT, N_OBS, MAX_OUTER, UID_BYTES, PEER_HANDLE_BYTES = 7, 9, 16, 128, 80

OK, NOT_ENOUGH_MAP_FEATURES, MAP_SEEDED = 0, 1, 2
SHARD_MAP, SHARD_QUERIES = 0, 1


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device_id", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
                ("max_iterations", C.c_int32), ("lm_max_iterations", C.c_int32), ("max_surface_features", C.c_int32),
                ("k", C.c_int32), ("tukey_variant", C.c_int32), ("time_kernels", C.c_int32),
                ("line_res", C.c_float), ("plane_res", C.c_float), ("yaw_ratio", C.c_double),
                ("velocity_failure_threshold", C.c_double), ("shard_mode", C.c_int32), ("solve_workgroups", C.c_int32)]


class IterStats(C.Structure):
    _fields_ = [("translation_norm", C.c_double), ("rotation_norm", C.c_double), ("num_surf_from_scan", C.c_int32),
                ("num_corner_from_scan", C.c_int32), ("lm_iterations", C.c_int32), ("num_successful_steps", C.c_int32),
                ("termination", C.c_int32), ("reserved", C.c_int32), ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("reject_hist", C.c_int32 * N_REJECT), ("obs_hist", C.c_int32 * N_OBS), ("pose_after", C.c_double * 7)]


class Stats(C.Structure):
    _fields_ = [("laser_cloud_surf_from_map_num", C.c_int32), ("laser_cloud_corner_from_map_num", C.c_int32),
                ("laser_cloud_surf_stack_num", C.c_int32), ("laser_cloud_corner_stack_num", C.c_int32),
                ("n_iterations", C.c_int32), ("startup_count", C.c_int32), ("pos_in_localmap", C.c_int32 * 3),
                ("prediction_source", C.c_int32), ("total_translation", C.c_double), ("total_rotation", C.c_double),
                ("translation_from_last", C.c_double), ("rotation_from_last", C.c_double), ("time_elapsed_ms", C.c_double),
                ("uncertainty", C.c_double * 6), ("JtJ", C.c_double * 36), ("Jtr", C.c_double * 6),
                ("iterations", IterStats * MAX_OUTER), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# so_icp_stats.flags
FLAG_PER_EVAL_LAUNCHES, FLAG_RETRIED, FLAG_HOST_MAP, FLAG_SORT_BINNING, FLAG_SHARDED, FLAG_STAGED_SCAN, FLAG_COPY_READBACK = 1, 2, 4, 8, 16, 32, 64
FLAG_QUERY_SPLIT = 128
FLAG_BINNED_AHEAD = 256
FLAG_QUERY_WAVES = 512
FLAG_CHAINED = 1024
FLAG_POSE_PRIOR = 2048
PRIOR_NONE, PRIOR_GIVEN, PRIOR_AT_GUESS = 0, 1, 2  # SO_ICP_PRIOR_*: the modes of so_icp_set_sequence_priors


class RegistrationError(C.Structure):
    """so_icp_registration_error_t (LidarSLAM::RegistrationError, LS.h:127-151)"""
    _fields_ = [("covariance", C.c_double * 36), ("position_error", C.c_double), ("position_error_direction", C.c_double * 3),
                ("pos_inverse_condition_num", C.c_double), ("orientation_error_deg", C.c_double),
                ("orientation_error_direction", C.c_double * 3), ("ori_inverse_condition_num", C.c_double)]


class PrefilterInfo(C.Structure):
    _fields_ = [("average_distance", C.c_double), ("count_far_points", C.c_int32), ("increase_blind_radius", C.c_int32),
                ("line_res", C.c_float), ("plane_res", C.c_float), ("statistic_in_input_order", C.c_int32), ("reserved", C.c_int32)]


class DeskewInfo(C.Structure):
    _fields_ = [("q_w_original_l", C.c_double * 4), ("t_w_original_l", C.c_double * 3), ("n_clamped", C.c_uint32), ("reserved", C.c_uint32)]


class SweepLayout(C.Structure):
    _fields_ = [("sensor", C.c_int32), ("is_bigendian", C.c_int32), ("point_step", C.c_uint32), ("row_step", C.c_uint32),
                ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32), ("off_intensity", C.c_int32), ("off_time", C.c_int32),
                ("off_ring", C.c_int32), ("filter_point_size", C.c_int32), ("min_range", C.c_float), ("T_ouster_sensor", C.c_double * 7)]


class FeatureInfo(C.Structure):
    _fields_ = [("q_w_original_l", C.c_double * 4), ("t_w_original_l", C.c_double * 3), ("n_clamped", C.c_uint32), ("deskewed", C.c_int32),
                ("n_points", C.c_uint64), ("n_surface", C.c_uint64)]


class LivoxLayout(C.Structure):
    """so_icp_livox_layout"""
    _fields_ = [("point_step", C.c_uint32), ("off_offset_time", C.c_int32), ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32),
                ("off_reflectivity", C.c_int32), ("off_tag", C.c_int32), ("off_line", C.c_int32), ("n_scans", C.c_int32),
                ("filter_point_size", C.c_int32), ("min_range", C.c_float), ("reserved", C.c_int32), ("R_imu_laser_gravity", C.c_double * 9)]


# livox_ros_driver2/msg/CustomPoint (uint32 offset_time; float32 x, y, z; uint8 reflectivity, tag, line): field -> byte offset
LIVOX_CUSTOM_POINT = {"offset_time": 0, "x": 4, "y": 8, "z": 12, "reflectivity": 16, "tag": 17, "line": 18}
LIVOX_POINT_STEP = 20  # points 20 bytes apart (CDR and C++ alike); the last field ends at byte 19


def livox_layout(filter_point_size=3, min_range=0.2, n_scans=4, R_imu_laser_gravity=None, point_step=LIVOX_POINT_STEP, offsets=None):
    """so_icp_livox_layout: so_icp_livox_default_layout (CustomPoint's offsets, the node's parameter defaults, R = identity) with
    the given values; offsets: field -> byte offset for another driver's point; R_imu_laser_gravity: 3 x 3, row-major."""
    L = LivoxLayout()
    load().so_icp_livox_default_layout(C.byref(L))
    L.point_step, L.n_scans, L.filter_point_size, L.min_range = int(point_step), int(n_scans), int(filter_point_size), float(min_range)
    for name, off in (offsets or {}).items():
        assert name in LIVOX_CUSTOM_POINT, name
        setattr(L, "off_" + name, int(off))
    if R_imu_laser_gravity is not None:
        for k, v in enumerate(np.asarray(R_imu_laser_gravity, np.float64).reshape(9)):
            L.R_imu_laser_gravity[k] = float(v)
    return L


class UntimedLayout(C.Structure):
    """so_icp_untimed_layout"""
    _fields_ = [("is_bigendian", C.c_int32), ("point_step", C.c_uint32), ("row_step", C.c_uint32), ("off_x", C.c_int32), ("off_y", C.c_int32),
                ("off_z", C.c_int32), ("off_intensity", C.c_int32), ("n_scans", C.c_int32), ("filter_point_size", C.c_int32),
                ("min_range", C.c_float)]


SENSOR_VELODYNE, SENSOR_OUSTER = 0, 1
# sensor_msgs::msg::PointField datatypes
INT8, UINT8, INT16, UINT16, INT32, UINT32, FLOAT32, FLOAT64 = range(1, 9)
# parameter.cpp:270-277: R = diag(-1, -1, 1) (the quaternion (0, 0, 1, 0)), t = (0, 0, 0.036180)
T_OUSTER_SENSOR = (0.0, 0.0, 0.036180, 0.0, 0.0, 1.0, 0.0)
# the fields pcl::fromROSMsg copies into the reference's point types: name -> (datatype, count)
_VELODYNE_FIELDS = {"x": FLOAT32, "y": FLOAT32, "z": FLOAT32, "intensity": FLOAT32, "time": FLOAT32, "ring": UINT16}   # PointcloudXYZITR
_OUSTER_FIELDS = {"x": FLOAT32, "y": FLOAT32, "z": FLOAT32, "intensity": FLOAT32, "t": UINT32}                          # OusterPointXYZIRT


def sweep_layout(fields, point_step, row_step, sensor, filter_point_size, min_range, is_bigendian=False, T_ouster_sensor=T_OUSTER_SENSOR):
    """so_icp_sweep_layout from a PointCloud2's PointField list [(name, offset, datatype, count), ...].  A field of the target point
    type is taken from the first PointField with its name, datatype and count (count 0 also matches a single value), as
    pcl::detail::FieldMatches does; a field with no match is absent (offset -1) and reads 0."""
    want = _OUSTER_FIELDS if sensor == SENSOR_OUSTER else _VELODYNE_FIELDS
    off = {}
    for name, dtype in want.items():
        for fname, foff, fdt, fcount in fields:
            if fname == name and fdt == dtype and (fcount == 1 or fcount == 0):
                off[name] = int(foff)
                break
    L = SweepLayout()
    L.sensor, L.is_bigendian, L.point_step, L.row_step = int(sensor), int(bool(is_bigendian)), int(point_step), int(row_step)
    L.off_x, L.off_y, L.off_z = off.get("x", -1), off.get("y", -1), off.get("z", -1)
    L.off_intensity = off.get("intensity", -1)
    L.off_time = off.get("t" if sensor == SENSOR_OUSTER else "time", -1)
    L.off_ring = -1 if sensor == SENSOR_OUSTER else off.get("ring", -1)
    L.filter_point_size, L.min_range = int(filter_point_size), float(min_range)
    for k in range(7):
        L.T_ouster_sensor[k] = float(T_ouster_sensor[k])
    return L


def untimed_layout(fields, point_step, row_step, n_scans, filter_point_size, min_range, is_bigendian=False):
    """so_icp_untimed_layout (a sweep without per-point time, assignTimeforPointCloud) from a PointCloud2's PointField list
    [(name, offset, datatype, count), ...]: pcl::PointXYZI's x y z intensity, matched as in sweep_layout (FLOAT32, count 1 or 0; a
    field with no match is absent and reads 0)."""
    off = {}
    for name in ("x", "y", "z", "intensity"):
        for fname, foff, fdt, fcount in fields:
            if fname == name and fdt == FLOAT32 and (fcount == 1 or fcount == 0):
                off[name] = int(foff)
                break
    L = UntimedLayout()
    L.is_bigendian, L.point_step, L.row_step = int(bool(is_bigendian)), int(point_step), int(row_step)
    L.off_x, L.off_y, L.off_z, L.off_intensity = off.get("x", -1), off.get("y", -1), off.get("z", -1), off.get("intensity", -1)
    L.n_scans, L.filter_point_size, L.min_range = int(n_scans), int(filter_point_size), float(min_range)
    return L


class Timing(C.Structure):
    _fields_ = [("knn_ms_total", C.c_double), ("knn_launches", C.c_int64), ("knn_queries", C.c_int64), ("knn_map_points", C.c_int64),
                ("eval_ms_total", C.c_double), ("eval_launches", C.c_int64), ("eval_points", C.c_int64),
                ("prep_ms_total", C.c_double), ("prep_launches", C.c_int64),
                ("host_ms_total", C.c_double), ("registrations", C.c_int64),
                ("knn_group_passes", C.c_int64), ("knn_fallback_lanes", C.c_int64), ("knn_candidates_scanned", C.c_int64),
                ("stage_wait_ms_total", C.c_double), ("staged_direct", C.c_int64), ("staged_copied", C.c_int64), ("stage_declined", C.c_int64),
                ("knn_packed_rows", C.c_int64), ("knn_packed_rows_too_many_runs", C.c_int64), ("knn_packed_rows_tile_full", C.c_int64),
                ("knn_packed_kept", C.c_int64), ("knn_pack_registrations", C.c_int64), ("knn_pack_holds", C.c_int64),
                ("seq_chained", C.c_int64), ("seq_chain_breaks", C.c_int64)]


class Sums(C.Structure):
    _fields_ = [("cost", C.c_double), ("count", C.c_double), ("Jtr", C.c_double * 6), ("JtJ", C.c_double * 21), ("hist", C.c_double * 16)]


class LmState(C.Structure):
    _fields_ = [("opaque", C.c_double * 96)]


class LmScriptEntry(C.Structure):
    _fields_ = [("sums", Sums), ("new_solve", C.c_int32), ("reserved", C.c_int32)]


class LmScriptStep(C.Structure):
    _fields_ = [("more", C.c_int32), ("reserved", C.c_int32), ("pose", C.c_double * 7), ("hand", (C.c_uint32 * 4) * 8), ("state", LmState)]


class LmScriptResult(C.Structure):
    _fields_ = [("state", LmState), ("T", C.c_double * 7), ("eval_pose", C.c_double * 7), ("T_final", C.c_double * 7),
                ("JtJ", C.c_double * 36), ("Jtr", C.c_double * 6),
                ("lm_more", C.c_int32), ("outer_iter", C.c_int32), ("n_iterations", C.c_int32), ("reg_done", C.c_int32),
                ("done_count", C.c_uint32), ("reserved", C.c_uint32), ("iterations", IterStats * 16)]


class Correspondence(C.Structure):
    """so_icp_correspondence: one accepted correspondence of the last outer iteration (72 bytes)"""
    _fields_ = [("index", C.c_uint32), ("p", C.c_float * 3), ("n", C.c_double * 3), ("d", C.c_double), ("coeff", C.c_double),
                ("residual", C.c_double), ("weight", C.c_double)]


class CorrespondenceInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_accepted", C.c_uint64), ("valid", C.c_int32), ("outer_iteration", C.c_int32),
                ("pose_fit", C.c_double * 7), ("pose_eval", C.c_double * 7), ("cost", C.c_double)]


class CorrespondenceGeometry(C.Structure):
    """so_icp_correspondence_geometry_record: neighbours, PCA and observability labels of one accepted correspondence (192 bytes)"""
    _fields_ = [("index", C.c_uint32), ("nbr_index", C.c_uint32 * 5), ("obs", C.c_uint8 * 3), ("reserved", C.c_uint8), ("nbr", C.c_float * 15),
                ("d2", C.c_float * 5), ("pad", C.c_uint32), ("pw", C.c_double * 3), ("eig", C.c_double * 3), ("pca_normal", C.c_double * 3),
                ("mean_abs_dist", C.c_double)]


class CorrespondenceGeometryInfo(C.Structure):
    _fields_ = [("n_points", C.c_uint64), ("n_accepted", C.c_uint64), ("valid", C.c_int32), ("outer_iteration", C.c_int32),
                ("pose_fit", C.c_double * 7), ("obs_hist", C.c_int32 * 9), ("reserved", C.c_int32)]


class PosePrior(C.Structure):
    """so_icp_pose_prior: T_meas {t, q = x y z w}, row-major U (residual = U e), the count scaling of the rows (all zero: U as given)"""
    _fields_ = [("T_meas", C.c_double * 7), ("sqrt_information", C.c_double * 36), ("count_floor", C.c_double * 6), ("count_fraction", C.c_double * 6)]


def pose_prior(T_meas, sqrt_information, count_floor=None, count_fraction=None):
    """a PosePrior from arrays: T_meas[7], U[6, 6] or [36], count_floor[6], count_fraction[6] (None: zeros)"""
    p = PosePrior()
    p.T_meas[:] = [float(v) for v in np.asarray(T_meas, dtype=np.float64).ravel()]
    p.sqrt_information[:] = [float(v) for v in np.asarray(sqrt_information, dtype=np.float64).ravel()]
    if count_floor is not None:
        p.count_floor[:] = [float(v) for v in count_floor]
    if count_fraction is not None:
        p.count_fraction[:] = [float(v) for v in count_fraction]
    return p


def pose_prior_from_information(information, T_meas):
    """so_icp_pose_prior_from_information: U = L^T of the LLT of `information` [6, 6] -> (rc, PosePrior)"""
    info = np.ascontiguousarray(information, dtype=np.float64).reshape(36)
    T = np.ascontiguousarray(T_meas, dtype=np.float64).reshape(7)
    out = PosePrior()
    rc = load().so_icp_pose_prior_from_information(_p(info, C.c_double), _p(T, C.c_double), C.byref(out))
    return rc, out


def pose_prior_sums(prior, pose, sums):
    """so_icp_pose_prior_sums: adds the prior at `pose` to `sums` (a Sums, in place); returns it"""
    pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(7)
    rc = load().so_icp_pose_prior_sums(C.byref(prior), _p(pose, C.c_double), C.byref(sums))
    if rc:
        raise SoIcpError(f"so_icp_pose_prior_sums: {rc}")
    return sums


# the same record as a numpy structured type (np.frombuffer over so_icp_correspondence bytes)
CORRESPONDENCE_DTYPE = np.dtype([("index", "<u4"), ("p", "<f4", 3), ("n", "<f8", 3), ("d", "<f8"), ("coeff", "<f8"), ("residual", "<f8"),
                                 ("weight", "<f8")])
assert CORRESPONDENCE_DTYPE.itemsize == C.sizeof(Correspondence) == 72
CORRESPONDENCE_GEOMETRY_DTYPE = np.dtype([("index", "<u4"), ("nbr_index", "<u4", 5), ("obs", "u1", 3), ("reserved", "u1"), ("nbr", "<f4", 15), ("d2", "<f4", 5),
                                          ("pad", "<u4"), ("pw", "<f8", 3), ("eig", "<f8", 3), ("pca_normal", "<f8", 3), ("mean_abs_dist", "<f8")])
assert CORRESPONDENCE_GEOMETRY_DTYPE.itemsize == C.sizeof(CorrespondenceGeometry) == 192

EXPORTED = ["so_icp_default_config", "so_icp_create", "so_icp_destroy", "so_icp_last_error", "so_icp_abi_version",
            "so_icp_device_available", "so_icp_set_resolution", "so_icp_set_max_surface_features", "so_icp_set_max_iterations",
            "so_icp_map_set_origin", "so_icp_map_shift", "so_icp_map_add_surf", "so_icp_map_count_5x5", "so_icp_map_export",
            "so_icp_map_size", "so_icp_map_clear", "so_icp_map_get_origin", "so_icp_knn_surf", "so_icp_register",
            "so_icp_register_dev", "so_icp_upload_scan", "so_icp_free_scan", "so_icp_localization", "so_icp_comm_unique_id", "so_icp_comm_init",
            "so_icp_shard_owner_of_point", "so_icp_cells_per_cube", "so_icp_lm_begin", "so_icp_lm_feed", "so_icp_lm_result",
            "so_icp_get_timing", "so_icp_reset_timing", "so_icp_set_time_kernels", "so_icp_synchronize", "so_icp_debug_stamps", "so_icp_debug_knn_stamps", "so_icp_register_batch", "so_icp_registration_error",
            "so_icp_localization_dev", "so_icp_download_scan", "so_icp_prefilter_scan", "so_icp_stage_scan", "so_icp_debug_match_status", "so_icp_comm_init_inprocess", "so_icp_peer_export", "so_icp_peer_connect", "so_icp_peer_enable",
            "so_icp_deskew_scan", "so_icp_deskew_scan_dev", "so_icp_transform_cloud", "so_icp_shard_histogram",
            "so_icp_host_register", "so_icp_host_unregister", "so_icp_host_alloc", "so_icp_host_free", "so_icp_device_count", "so_icp_stage_cancel",
            "so_icp_map_insert_stats", "so_icp_register_sequence", "so_icp_map_export_records", "so_icp_sequence_announce_next", "so_icp_debug_neighbours", "so_icp_prefilter_announce",
            "so_icp_localization_sequence", "so_icp_extract_features", "so_icp_extract_features_dev", "so_icp_prefilter_scan_dev",
            "so_icp_livox_default_layout", "so_icp_extract_features_livox", "so_icp_extract_features_livox_dev",
            "so_icp_registered_scan", "so_icp_registered_scan_dev", "so_icp_extract_features_untimed", "so_icp_extract_features_untimed_dev",
            "so_icp_debug_lm_script", "so_icp_set_cloud_intensity", "so_icp_prefilter_intensity",
            "so_icp_keep_correspondences", "so_icp_correspondences",
            "so_icp_match", "so_icp_match_dev", "so_icp_match_batch", "so_icp_correspondence_sums",
            "so_icp_keep_correspondence_geometry", "so_icp_correspondence_geometry", "so_icp_debug_correspondence_refit",
            "so_icp_pose_prior_from_information", "so_icp_pose_prior_sums", "so_icp_set_pose_prior", "so_icp_set_sequence_priors",
            "so_icp_set_batch_priors",
            "so_icp_keep_sequence_correspondences", "so_icp_sequence_correspondences", "so_icp_sequence_correspondence_sums",
            "so_icp_keep_batch_correspondences", "so_icp_batch_correspondences", "so_icp_batch_correspondence_sums"]
SUMS_MAX_POSES = 64
BATCH_MAX_SELECTION = 1024
SEQUENCE_MAX_SELECTION = 1024

_lib = None


def load():
    """Load libsoicp.so; raise if it is absent (run `python -m superodom_amd.build`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not built: run `python -m superodom_amd.build` (hipcc, gfx950). "
                           "superodom_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, f32p, f64p, i32p = C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    u8p = C.POINTER(C.c_uint8)
    L.so_icp_default_config.argtypes = [C.POINTER(Config)]; L.so_icp_default_config.restype = None
    L.so_icp_create.argtypes = [C.POINTER(Config)]; L.so_icp_create.restype = vp
    L.so_icp_destroy.argtypes = [vp]; L.so_icp_destroy.restype = None
    L.so_icp_last_error.argtypes = [vp]; L.so_icp_last_error.restype = C.c_char_p
    L.so_icp_set_resolution.argtypes = [vp, C.c_float, C.c_float]
    L.so_icp_set_max_surface_features.argtypes = [vp, C.c_int]
    L.so_icp_set_max_iterations.argtypes = [vp, C.c_int]
    L.so_icp_set_cloud_intensity.argtypes = [vp, C.c_int]
    L.so_icp_prefilter_intensity.argtypes = [vp, f32p, C.c_size_t, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.so_icp_map_set_origin.argtypes = [vp, f64p, i32p]
    L.so_icp_map_shift.argtypes = [vp, f64p, i32p]
    L.so_icp_map_add_surf.argtypes = [vp, f32p, C.c_size_t, C.c_size_t]
    L.so_icp_map_count_5x5.argtypes = [vp, i32p, i32p, i32p]
    L.so_icp_map_export.argtypes = [vp, f32p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, i32p]
    L.so_icp_map_size.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.so_icp_map_export_records.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_size_t), C.c_int, i32p]
    L.so_icp_map_clear.argtypes = [vp]
    L.so_icp_map_insert_stats.argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.so_icp_map_get_origin.argtypes = [vp, i32p]
    L.so_icp_knn_surf.argtypes = [vp, f32p, C.c_size_t, C.c_int, f32p, f32p, i32p, u8p]
    L.so_icp_register.argtypes = [vp, f32p, C.c_size_t, C.c_size_t, f64p, f64p, C.POINTER(Stats)]
    L.so_icp_register_dev.argtypes = [vp, vp, C.c_size_t, f64p, f64p, C.POINTER(Stats)]
    L.so_icp_sequence_announce_next.argtypes = [vp, f32p, C.c_size_t, f64p]
    L.so_icp_register_sequence.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_int, f64p, f64p, f64p, f64p, C.POINTER(Stats), i32p]
    L.so_icp_localization_sequence.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), C.c_size_t, C.c_int, f64p, f64p, f64p, f64p, f64p,
                                               C.POINTER(Stats), i32p]
    L.so_icp_upload_scan.argtypes = [vp, f32p, C.c_size_t, C.c_size_t, C.POINTER(vp)]
    L.so_icp_free_scan.argtypes = [vp, vp]
    L.so_icp_localization.argtypes = [vp, C.c_int, f64p, f32p, C.c_size_t, C.c_size_t, C.c_double, f64p, C.POINTER(Stats)]
    L.so_icp_comm_unique_id.argtypes = [u8p]
    L.so_icp_comm_init.argtypes = [vp, u8p]
    L.so_icp_shard_owner_of_point.argtypes = [f32p, i32p, C.c_float, C.c_int]
    L.so_icp_cells_per_cube.argtypes = [C.c_float, f64p]
    L.so_icp_shard_histogram.argtypes = [f32p, C.c_size_t, C.c_size_t, f64p, i32p, C.c_float, C.c_int, C.POINTER(C.c_int64)]
    L.so_icp_lm_begin.argtypes = [C.POINTER(LmState), f64p, C.POINTER(Sums), C.c_int, f64p]
    L.so_icp_lm_feed.argtypes = [C.POINTER(LmState), C.POINTER(Sums), f64p]
    L.so_icp_lm_result.argtypes = [C.POINTER(LmState), f64p, C.POINTER(IterStats)]
    L.so_icp_get_timing.argtypes = [vp, C.POINTER(Timing)]
    L.so_icp_reset_timing.argtypes = [vp]
    L.so_icp_synchronize.argtypes = [vp]
    L.so_icp_debug_stamps.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.so_icp_register_batch.argtypes = [vp, f32p, vp, C.c_size_t, C.c_size_t, f64p, C.c_int, f64p, C.POINTER(Stats), i32p]
    L.so_icp_registration_error.argtypes = [C.POINTER(Stats), C.POINTER(RegistrationError)]
    L.so_icp_localization_dev.argtypes = [vp, C.c_int, f64p, vp, C.c_size_t, C.c_double, f64p, C.POINTER(Stats)]
    L.so_icp_download_scan.argtypes = [vp, vp, C.c_size_t, f32p]
    for fn in (L.so_icp_deskew_scan, L.so_icp_deskew_scan_dev):
        fn.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_double, C.POINTER(C.c_double), C.c_size_t, C.c_int, C.POINTER(C.c_double),
                       C.POINTER(DeskewInfo)]
    L.so_icp_transform_cloud.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.POINTER(C.c_size_t)]
    L.so_icp_registered_scan.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), vp, C.POINTER(C.c_size_t)]
    L.so_icp_registered_scan_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.POINTER(C.c_double), vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.so_icp_prefilter_announce.argtypes = [vp, f32p, C.c_size_t, C.c_size_t]
    L.so_icp_prefilter_scan.argtypes = [vp, f32p, C.c_size_t, C.c_size_t, C.c_int, C.c_float, C.c_float, C.POINTER(vp),
                                        C.POINTER(C.c_size_t), C.POINTER(PrefilterInfo)]
    L.so_icp_prefilter_scan_dev.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_float, C.c_float, C.POINTER(vp),
                                            C.POINTER(C.c_size_t), C.POINTER(PrefilterInfo)]
    L.so_icp_extract_features.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(SweepLayout), C.c_double, C.POINTER(C.c_double), C.c_size_t,
                                          C.c_int, C.POINTER(C.c_double), vp, vp, C.POINTER(FeatureInfo)]
    L.so_icp_extract_features_dev.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(SweepLayout), C.c_double, C.POINTER(C.c_double),
                                              C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(vp), C.POINTER(vp), C.POINTER(FeatureInfo)]
    L.so_icp_livox_default_layout.argtypes = [C.POINTER(LivoxLayout)]; L.so_icp_livox_default_layout.restype = None
    L.so_icp_extract_features_livox.argtypes = [vp, vp, C.c_uint32, C.POINTER(LivoxLayout), C.c_double, C.POINTER(C.c_double), C.c_size_t,
                                                C.c_int, C.POINTER(C.c_double), vp, vp, C.POINTER(FeatureInfo)]
    L.so_icp_extract_features_livox_dev.argtypes = [vp, vp, C.c_uint32, C.POINTER(LivoxLayout), C.c_double, C.POINTER(C.c_double), C.c_size_t,
                                                    C.c_int, C.POINTER(C.c_double), C.POINTER(vp), C.POINTER(vp), C.POINTER(FeatureInfo)]
    L.so_icp_extract_features_untimed.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(UntimedLayout), C.c_double, C.POINTER(C.c_double),
                                                  C.c_size_t, C.c_int, C.POINTER(C.c_double), vp, vp, C.POINTER(FeatureInfo)]
    L.so_icp_extract_features_untimed_dev.argtypes = [vp, vp, C.c_uint32, C.c_uint32, C.POINTER(UntimedLayout), C.c_double, C.POINTER(C.c_double),
                                                      C.c_size_t, C.c_int, C.POINTER(C.c_double), C.POINTER(vp), C.POINTER(vp), C.POINTER(FeatureInfo)]
    L.so_icp_debug_knn_stamps.argtypes = [vp, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t)]
    L.so_icp_set_time_kernels.argtypes = [vp, C.c_int]
    L.so_icp_stage_scan.argtypes = [vp, f32p, C.c_size_t, C.c_size_t]
    L.so_icp_host_register.argtypes = [vp, vp, C.c_size_t]
    L.so_icp_stage_cancel.argtypes = [vp, f32p]
    L.so_icp_host_unregister.argtypes = [vp, vp]
    L.so_icp_host_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.so_icp_host_free.argtypes = [vp, vp]
    L.so_icp_debug_match_status.argtypes = [vp, u8p, C.c_size_t]
    L.so_icp_debug_neighbours.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t]
    L.so_icp_debug_lm_script.argtypes = [vp, C.c_int, f64p, C.c_int, C.c_int, C.c_int, C.POINTER(LmScriptEntry), C.c_int, C.c_uint64,
                                         C.POINTER(LmScriptStep), C.POINTER(LmScriptResult)]
    L.so_icp_comm_init_inprocess.argtypes = [vp, C.c_uint64]
    L.so_icp_peer_export.argtypes = [vp, u8p]
    L.so_icp_peer_connect.argtypes = [vp, u8p, i32p]
    L.so_icp_peer_enable.argtypes = [vp, C.c_int]
    L.so_icp_keep_correspondences.argtypes = [vp, C.c_int]
    L.so_icp_correspondences.argtypes = [vp, f64p, vp, C.c_size_t, u8p, f32p, C.c_size_t, C.POINTER(vp), C.POINTER(CorrespondenceInfo)]
    L.so_icp_match.argtypes = [vp, f32p, C.c_size_t, C.c_size_t, f64p, C.POINTER(Stats)]
    L.so_icp_match_dev.argtypes = [vp, vp, C.c_size_t, f64p, C.POINTER(Stats)]
    L.so_icp_match_batch.argtypes = [vp, f32p, vp, C.c_size_t, C.c_size_t, f64p, C.c_int, C.POINTER(Stats), i32p]
    L.so_icp_correspondence_sums.argtypes = [vp, f64p, C.c_int, C.POINTER(Sums)]
    L.so_icp_keep_correspondence_geometry.argtypes = [vp, C.c_int]
    L.so_icp_correspondence_geometry.argtypes = [vp, vp, C.c_size_t, u8p, C.c_size_t, C.POINTER(vp), C.POINTER(CorrespondenceGeometryInfo)]
    L.so_icp_debug_correspondence_refit.argtypes = [vp, f64p, C.c_size_t, C.POINTER(C.c_size_t)]
    L.so_icp_pose_prior_from_information.argtypes = [f64p, f64p, C.POINTER(PosePrior)]
    L.so_icp_pose_prior_sums.argtypes = [C.POINTER(PosePrior), f64p, C.POINTER(Sums)]
    L.so_icp_set_pose_prior.argtypes = [vp, C.POINTER(PosePrior)]
    L.so_icp_set_sequence_priors.argtypes = [vp, C.c_int, C.POINTER(PosePrior), C.POINTER(C.c_uint8)]
    L.so_icp_set_batch_priors.argtypes = [vp, C.c_int, C.POINTER(PosePrior), C.POINTER(C.c_uint8)]
    L.so_icp_keep_batch_correspondences.argtypes = [vp, C.c_int]
    L.so_icp_batch_correspondences.argtypes = [vp, i32p, C.c_int, f64p, vp, C.c_size_t, C.POINTER(C.c_uint64), u8p, C.c_size_t, C.POINTER(vp),
                                               C.POINTER(CorrespondenceInfo)]
    L.so_icp_batch_correspondence_sums.argtypes = [vp, i32p, C.c_int, f64p, C.c_int, C.POINTER(Sums)]
    L.so_icp_keep_sequence_correspondences.argtypes = [vp, C.c_int]
    L.so_icp_sequence_correspondences.argtypes = [vp, i32p, C.c_int, f64p, vp, C.c_size_t, C.POINTER(C.c_uint64), u8p, C.c_size_t, C.POINTER(C.c_uint64),
                                                  C.POINTER(vp), C.POINTER(CorrespondenceInfo)]
    L.so_icp_sequence_correspondence_sums.argtypes = [vp, i32p, C.c_int, f64p, C.c_int, C.POINTER(Sums)]
    _lib = L
    return L


_F64P = C.POINTER(C.c_double)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def default_config(**kw):
    cfg = Config()
    load().so_icp_default_config(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


class SoIcpError(RuntimeError):
    pass


class LidarSlamGpu:
    """Host-side mirror of the reference's LidarSLAM object for this path: owns one so_icp_ctx
    (= LidarSLAM::localMap + the ICP state), methods named after the reference members they replace."""

    def __init__(self, **cfg_kw):
        self.L = load()
        self.cfg = default_config(**cfg_kw)
        self.h = self.L.so_icp_create(C.byref(self.cfg))
        if not self.h:
            raise SoIcpError(self.L.so_icp_last_error(None).decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.so_icp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc < 0:
            raise SoIcpError(f"so_icp error {rc}: {self.L.so_icp_last_error(self.h).decode()}")
        return rc

    # ---- LocalMap ----
    def set_resolution(self, line_res, plane_res):
        self._check(self.L.so_icp_set_resolution(self.h, line_res, plane_res))

    def set_max_surface_features(self, n):
        self._check(self.L.so_icp_set_max_surface_features(self.h, int(n)))

    def set_max_iterations(self, n):
        self._check(self.L.so_icp_set_max_iterations(self.h, int(n)))

    def set_origin(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64); o = np.zeros(3, np.int32)
        self._check(self.L.so_icp_map_set_origin(self.h, _p(t, C.c_double), _p(o, C.c_int32)))
        return o

    def origin(self):
        o = np.zeros(3, np.int32); self._check(self.L.so_icp_map_get_origin(self.h, _p(o, C.c_int32))); return o

    def shift_map(self, t):
        t = np.ascontiguousarray(t, dtype=np.float64); o = np.zeros(3, np.int32)
        self._check(self.L.so_icp_map_shift(self.h, _p(t, C.c_double), _p(o, C.c_int32)))
        return o

    def add_surf_point_cloud(self, xyz):
        xyz = _f32(xyz).reshape(-1, 3)
        return self._check(self.L.so_icp_map_add_surf(self.h, _p(xyz, C.c_float), len(xyz), 12))

    def set_cloud_intensity(self, offset_bytes):
        """so_icp_set_cloud_intensity: byte offset of the FLOAT32 intensity in a point record (16: pcl::PointXYZI), -1: off.
        Returns the C code (negative: refused) -- it does not raise."""
        return self.L.so_icp_set_cloud_intensity(self.h, int(offset_bytes))

    def add_surf_records(self, records):
        """so_icp_map_add_surf on records: float32 array (n, w), x y z in the first three columns, stride 4 w bytes"""
        rec = _f32(records); assert rec.ndim == 2 and rec.shape[1] >= 3
        return self._check(self.L.so_icp_map_add_surf(self.h, _p(rec, C.c_float), len(rec), 4 * rec.shape[1]))

    def count_5x5(self, pos):
        pos = np.ascontiguousarray(pos, dtype=np.int32); ne = C.c_int32(); ns = C.c_int32()
        self._check(self.L.so_icp_map_count_5x5(self.h, _p(pos, C.c_int32), C.byref(ne), C.byref(ns)))
        return ns.value

    def map_size(self, this_rank=False):
        n = C.c_size_t(); nr = C.c_size_t()
        self._check(self.L.so_icp_map_size(self.h, C.byref(n), C.byref(nr) if this_rank else None))
        return (n.value, nr.value) if this_rank else n.value

    def export_map(self, only_5x5=False, pos=None):
        n = self.map_size(); out = np.zeros((max(n, 1), 3), np.float32); m = C.c_size_t()
        posa = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
        self._check(self.L.so_icp_map_export(self.h, _p(out, C.c_float), n, C.byref(m), int(only_5x5),
                                             None if posa is None else _p(posa, C.c_int32)))
        return out[:m.value].copy()

    def export_map_records(self, stride=32, only_5x5=False, pos=None, out=None):
        """so_icp_map_export_records: the map as records of `stride` bytes (x, y, z floats first, rest zero) -> uint8 array (n, stride)"""
        posa = None if pos is None else np.ascontiguousarray(pos, dtype=np.int32)
        pp = None if posa is None else _p(posa, C.c_int32)
        m = C.c_size_t()
        self._check(self.L.so_icp_map_export_records(self.h, None, stride, 0, C.byref(m), int(only_5x5), pp))
        n = m.value
        buf = out if out is not None else np.zeros((max(n, 1), stride), np.uint8)
        assert buf.nbytes >= n * stride
        self._check(self.L.so_icp_map_export_records(self.h, buf.ctypes.data_as(C.c_void_p), stride, n, C.byref(m), int(only_5x5), pp))
        return buf.reshape(-1)[:m.value * stride].reshape(m.value, stride)

    def clear_map(self):
        self._check(self.L.so_icp_map_clear(self.h))

    def map_insert_stats(self):
        """(inserts laid out by the device, of those handed back to the host's round-by-round path)"""
        a = C.c_uint(); b = C.c_uint()
        self._check(self.L.so_icp_map_insert_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- Seam B ----
    def nearest_k_search_surf(self, q, k=5, want_index=True):
        q = _f32(q).reshape(-1, 3); nq = len(q)
        nbr = np.zeros((nq, k, 3), np.float32); d2 = np.zeros((nq, k), np.float32)
        idx = np.zeros((nq, k), np.int32); found = np.zeros(nq, np.uint8)
        self._check(self.L.so_icp_knn_surf(self.h, _p(q, C.c_float), nq, k, _p(nbr, C.c_float), _p(d2, C.c_float),
                                           _p(idx, C.c_int32) if want_index else None, _p(found, C.c_uint8)))
        return found, nbr, d2, idx

    # ---- Seam A ----
    def register(self, scan, pose_in):
        scan = _f32(scan).reshape(-1, 3); pose_in = np.ascontiguousarray(pose_in, dtype=np.float64)
        out = np.zeros(7); st = Stats()
        rc = self._check(self.L.so_icp_register(self.h, _p(scan, C.c_float), len(scan), 12, _p(pose_in, C.c_double),
                                                _p(out, C.c_double), C.byref(st)))
        return rc, out, st

    def stage_scan(self, scan):
        """so_icp_stage_scan: announce the NEXT scan (contiguous float32 (n,3) array that stays alive and unchanged until
        the register call that consumes it)."""
        assert isinstance(scan, np.ndarray) and scan.dtype == np.float32 and scan.flags.c_contiguous
        self._check(self.L.so_icp_stage_scan(self.h, _p(scan, C.c_float), len(scan), 12))

    def stage_cancel(self, scan):
        self._check(self.L.so_icp_stage_cancel(self.h, _p(scan, C.c_float)))

    def host_register(self, arr):
        """so_icp_host_register: pin the numpy array's memory (it must stay alive until host_unregister / close); packed scans
        announced from inside it travel to HBM by DMA straight from the array."""
        assert isinstance(arr, np.ndarray) and arr.flags.c_contiguous
        self._check(self.L.so_icp_host_register(self.h, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def host_alloc_like(self, arr):
        """A copy of `arr` in pinned host memory from so_icp_host_alloc (numpy view; valid until close())."""
        arr = np.ascontiguousarray(arr)
        p = C.c_void_p()
        self._check(self.L.so_icp_host_alloc(self.h, arr.nbytes, C.byref(p)))
        buf = (C.c_char * arr.nbytes).from_address(p.value)
        out = np.frombuffer(buf, dtype=arr.dtype).reshape(arr.shape)
        out[...] = arr
        return out

    def host_unregister(self, arr):
        self._check(self.L.so_icp_host_unregister(self.h, arr.ctypes.data_as(C.c_void_p)))

    def prepare_stage_scan(self, scan):
        assert isinstance(scan, np.ndarray) and scan.dtype == np.float32 and scan.flags.c_contiguous
        fn, args = self.L.so_icp_stage_scan, (self.h, _p(scan, C.c_float), len(scan), 12)
        return lambda: fn(*args)

    def prepare_register(self, scan, pose_in, stats, pose_out):
        """Zero-argument callable performing one so_icp_register (host scan buffer) with pre-built ctypes arguments."""
        assert isinstance(scan, np.ndarray) and scan.dtype == np.float32 and scan.flags.c_contiguous
        assert pose_in.dtype == np.float64 and pose_in.flags.c_contiguous and pose_out.dtype == np.float64 and pose_out.flags.c_contiguous
        fn, args = self.L.so_icp_register, (self.h, _p(scan, C.c_float), len(scan), 12, pose_in.ctypes.data_as(_F64P),
                                            pose_out.ctypes.data_as(_F64P), C.byref(stats))
        return lambda: fn(*args)

    def match_status(self, n):
        """MatchingResult of every query of the last registration's last outer iteration (so_icp_debug_match_status)."""
        out = np.zeros(n, np.uint8)
        self._check(self.L.so_icp_debug_match_status(self.h, _p(out, C.c_uint8), n))
        return out

    def keep_correspondences(self, on):
        """so_icp_keep_correspondences: registrations from here on leave their correspondence set for correspondences(); returns the C code"""
        return self.L.so_icp_keep_correspondences(self.h, int(bool(on)))

    def _correspondences(self, pose, want_points, cap, want_records, d_out):
        pose = None if pose is None else np.ascontiguousarray(pose, np.float64)
        info = CorrespondenceInfo()
        if cap is None:  # a sizing call first (counts only): one launch more than a call with `cap`
            self._check(self.L.so_icp_correspondences(self.h, None, None, 0, None, None, 0, None, C.byref(info)))
            cap = int(info.n_points)
        cap = int(cap)
        rec = np.zeros(cap if want_records else 0, CORRESPONDENCE_DTYPE)
        status = np.zeros(cap, np.uint8) if want_points else None
        resid = np.zeros(cap, np.float32) if want_points else None
        self._check(self.L.so_icp_correspondences(self.h, None if pose is None else _p(pose, C.c_double),
                                                  rec.ctypes.data_as(C.c_void_p) if want_records else None, len(rec),
                                                  None if status is None else _p(status, C.c_uint8), None if resid is None else _p(resid, C.c_float),
                                                  cap if want_points else 0, d_out, C.byref(info)))
        n, na = int(info.n_points), int(info.n_accepted)
        return rec[:na], (None if status is None else status[:n]), (None if resid is None else resid[:n]), info

    def correspondences(self, pose=None, want_points=True, cap=None):
        """so_icp_correspondences: the accepted correspondences of the last registration as a structured array (CORRESPONDENCE_DTYPE,
        ascending index), the status byte and the float residual (NaN where not accepted) of every scan point (None without
        want_points) and the CorrespondenceInfo.  pose: where residual, weight and cost are evaluated (None: the optimised pose).
        cap: an upper bound of the scan's points, when the caller knows one (saves the sizing call).  info.valid == 0: empty arrays."""
        return self._correspondences(pose, want_points, cap, True, None)

    def prepare_correspondences(self, cap, want_points=True):
        """so_icp_correspondences at the default pose with pre-built arguments and buffers for `cap` points (timed loops).  Returns
        (call, records, status or None, residual or None, info): call() performs the C call and returns its code; the first
        info.n_accepted records and info.n_points per-point entries are then current."""
        rec = np.zeros(int(cap), CORRESPONDENCE_DTYPE); info = CorrespondenceInfo()
        status = np.zeros(int(cap), np.uint8) if want_points else None
        resid = np.zeros(int(cap), np.float32) if want_points else None
        fn, args = self.L.so_icp_correspondences, (self.h, None, rec.ctypes.data_as(C.c_void_p), len(rec), None if status is None else _p(status, C.c_uint8),
                                                   None if resid is None else _p(resid, C.c_float), int(cap) if want_points else 0, None, C.byref(info))
        return (lambda: fn(*args)), rec, status, resid, info

    def correspondences_dev(self, pose=None, cap=None):
        """the same, the records left in HBM: (device address of the context-owned record buffer -- valid until the next call --, info)"""
        d = C.c_void_p()
        _, _, _, info = self._correspondences(pose, False, 0 if cap is None else cap, False, C.byref(d))
        return d.value, info

    # ---- the geometry of the kept set: neighbours, PCA, observability labels ----
    def keep_correspondence_geometry(self, on):
        """so_icp_keep_correspondence_geometry: registrations from here on also leave the snapshot correspondence_geometry() refits
        from (needs keep_correspondences(True)); returns the C code"""
        return self.L.so_icp_keep_correspondence_geometry(self.h, int(bool(on)))

    def _correspondence_geometry(self, cap, want_points, want_records, d_out):
        info = CorrespondenceGeometryInfo()
        if cap is None:  # a sizing call first (counts only): one launch more than a call with `cap`
            self._check(self.L.so_icp_correspondence_geometry(self.h, None, 0, None, 0, None, C.byref(info)))
            cap = int(info.n_points)
        cap = int(cap)
        rec = np.zeros(cap if want_records else 0, CORRESPONDENCE_GEOMETRY_DTYPE)
        labels = np.zeros((cap, 3), np.uint8) if want_points else None
        self._check(self.L.so_icp_correspondence_geometry(self.h, rec.ctypes.data_as(C.c_void_p) if want_records else None, len(rec),
                                                          None if labels is None else _p(labels, C.c_uint8), cap if want_points else 0, d_out, C.byref(info)))
        return rec[:int(info.n_accepted)], (None if labels is None else labels[:int(info.n_points)]), info

    def correspondence_geometry(self, cap=None, want_points=True):
        """so_icp_correspondence_geometry: one record (CORRESPONDENCE_GEOMETRY_DTYPE) per accepted correspondence of the last registration,
        ascending index, pairing with correspondences(); the three observability labels of every scan point ([n, 3] uint8, 255 where the
        point was not accepted; None without want_points) and the CorrespondenceGeometryInfo.  cap: an upper bound of the scan's points
        (saves the sizing call).  info.valid == 0: empty arrays."""
        return self._correspondence_geometry(cap, want_points, True, None)

    def correspondence_geometry_dev(self):
        """the same, the records left in HBM: (device address of the context-owned record buffer -- valid until the next call --, info)"""
        d = C.c_void_p()
        _, _, info = self._correspondence_geometry(0, False, False, C.byref(d))
        return d.value, info

    def prepare_correspondence_geometry(self, cap, want_points=True):
        """so_icp_correspondence_geometry with pre-built arguments and buffers for `cap` points (timed loops): (call, records, labels, info)"""
        rec = np.zeros(int(cap), CORRESPONDENCE_GEOMETRY_DTYPE); info = CorrespondenceGeometryInfo()
        labels = np.zeros((int(cap), 3), np.uint8) if want_points else None
        fn, args = self.L.so_icp_correspondence_geometry, (self.h, rec.ctypes.data_as(C.c_void_p), len(rec), None if labels is None else _p(labels, C.c_uint8),
                                                           int(cap) if want_points else 0, None, C.byref(info))
        return (lambda: fn(*args)), rec, labels, info

    def debug_correspondence_refit(self, cap):
        """so_icp_debug_correspondence_refit: the plane the geometry export refits per accepted point, [n_accepted, 5] = n[3], d, coeff"""
        out = np.zeros((int(cap), 5), np.float64); n = C.c_size_t()
        self._check(self.L.so_icp_debug_correspondence_refit(self.h, _p(out, C.c_double), int(cap), C.byref(n)))
        return out[:n.value]

    # ---- Seam C: the matching half at a pose of the caller's, and the kept set's sums on the device ----
    def match(self, scan, pose):
        """so_icp_match: one outer iteration's matching half and the evaluation at `pose` (needs keep_correspondences(True)); -> (rc, Stats)"""
        scan = _f32(scan).reshape(-1, 3); pose = np.ascontiguousarray(pose, dtype=np.float64)
        st = Stats()
        rc = self._check(self.L.so_icp_match(self.h, _p(scan, C.c_float), len(scan), 12, _p(pose, C.c_double), C.byref(st)))
        return rc, st

    def match_dev(self, d_scan, n, pose):
        pose = np.ascontiguousarray(pose, dtype=np.float64); st = Stats()
        rc = self._check(self.L.so_icp_match_dev(self.h, d_scan, n, _p(pose, C.c_double), C.byref(st)))
        return rc, st

    def match_batch(self, scan, poses, d_scan=None, n=None):
        """so_icp_match_batch: the same scan matched at many poses in one call, no solve.  scan: host array, or None with (d_scan, n) from
        upload_scan.  Returns (number of poses that ended SO_ICP_OK, rc[n_poses], stats list); with keep_batch_correspondences(True)
        the call leaves the batch's kept set (batch_correspondences / batch_correspondence_sums)."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        B = len(poses)
        rcs = np.zeros(B, np.int32); st = (Stats * max(B, 1))()
        if d_scan is None:
            scan = _f32(scan).reshape(-1, 3)
            ok = self._check(self.L.so_icp_match_batch(self.h, _p(scan, C.c_float), None, len(scan), 12, _p(poses, C.c_double), B, st, _p(rcs, C.c_int32)))
        else:
            ok = self._check(self.L.so_icp_match_batch(self.h, None, d_scan, n, 12, _p(poses, C.c_double), B, st, _p(rcs, C.c_int32)))
        return ok, rcs, list(st)[:B]

    def set_pose_prior(self, prior):
        """so_icp_set_pose_prior: `prior` (a PosePrior) goes into the next register / register_dev / localization(_dev) call and is consumed
        by it; None withdraws a pending one"""
        self._check(self.L.so_icp_set_pose_prior(self.h, C.byref(prior) if prior is not None else None))

    def _set_priors(self, setter, priors, modes):
        if priors is None or len(priors) == 0:
            self._check(setter(self.h, 0, None, None)); return
        arr = (PosePrior * len(priors))(*priors)
        m = None
        if modes is not None:
            assert len(modes) == len(priors)
            m = (C.c_uint8 * len(priors))(*[int(v) for v in modes])
        self._check(setter(self.h, len(priors), arr, m))

    def set_sequence_priors(self, priors, modes=None):
        """so_icp_set_sequence_priors: one PosePrior per frame of the next register_sequence / localization_sequence call, which consumes
        them; modes[k] in PRIOR_NONE / PRIOR_GIVEN / PRIOR_AT_GUESS (None: all given).  priors None or empty withdraws pending ones"""
        self._set_priors(self.L.so_icp_set_sequence_priors, priors, modes)

    def set_batch_priors(self, priors, modes=None):
        """so_icp_set_batch_priors: one PosePrior per hypothesis of the next register_batch call, which consumes them; modes[h] in
        PRIOR_NONE / PRIOR_GIVEN / PRIOR_AT_GUESS (None: all given; AT_GUESS: T_meas := poses_in[h] of that call).  priors None or
        empty withdraws pending ones"""
        self._set_priors(self.L.so_icp_set_batch_priors, priors, modes)

    def correspondence_sums(self, poses):
        """so_icp_correspondence_sums: the kept set's cost and normal equations at `poses` ([7] or [k, 7], k <= SUMS_MAX_POSES) -> an
        array of k Sums (what LmDriver.begin / feed take)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        out = (Sums * len(poses))()
        self._check(self.L.so_icp_correspondence_sums(self.h, _p(poses, C.c_double), len(poses), out))
        return out

    def prepare_correspondence_sums(self, poses):
        """the same with pre-built arguments (timed loops): (call, poses array the caller may rewrite in place, Sums array)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7).copy()
        out = (Sums * len(poses))()
        fn, args = self.L.so_icp_correspondence_sums, (self.h, poses.ctypes.data_as(_F64P), len(poses), out)
        return (lambda: fn(*args)), poses, out

    # ---- the correspondence sets of a batch's hypotheses ----
    def keep_batch_correspondences(self, on):
        """so_icp_keep_batch_correspondences: register_batch calls from here on leave the sets of all their hypotheses for
        batch_correspondences() / batch_correspondence_sums(); returns the C code"""
        return self.L.so_icp_keep_batch_correspondences(self.h, int(bool(on)))

    def batch_correspondences(self, hyp=None, n_sel=None, poses=None, want_status=True, cap_points=None, cap_records=None, want_records=True, d_out=None):
        """so_icp_batch_correspondences for the selection `hyp` (None: hypotheses 0 .. n_sel - 1) of the last batch, entry k evaluated at
        poses[k] (None: each hypothesis' own optimised pose).  -> (records of the whole selection (CORRESPONDENCE_DTYPE), first_record
        [n_sel + 1]: entry k's records are records[first_record[k]:first_record[k + 1]], status [n_sel, n_points] or None, the n_sel
        CorrespondenceInfo).  cap_points / cap_records: upper bounds of the scan's points / the selection's records, when the caller
        knows them (saves the sizing call)."""
        hyp = None if hyp is None else np.ascontiguousarray(hyp, np.int32)
        n_sel = len(hyp) if hyp is not None else int(n_sel)
        poses = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(n_sel, 7)
        hp = None if hyp is None else _p(hyp, C.c_int32)
        pp = None if poses is None else _p(poses, C.c_double)
        info = (CorrespondenceInfo * max(n_sel, 1))()
        first = np.zeros(n_sel + 1, np.uint64)
        if cap_points is None or (want_records and cap_records is None):  # a sizing call first (counts only): one launch more
            self._check(self.L.so_icp_batch_correspondences(self.h, hp, n_sel, pp, None, 0, _p(first, C.c_uint64), None, 0, None, info))
            cap_points = max([int(info[k].n_points) for k in range(n_sel)], default=0)
            cap_records = int(first[n_sel])
        cap_points, cap_records = int(cap_points), int(cap_records or 0)
        rec = np.zeros(cap_records if want_records else 0, CORRESPONDENCE_DTYPE)
        status = np.zeros(n_sel * cap_points, np.uint8) if want_status else None
        self._check(self.L.so_icp_batch_correspondences(self.h, hp, n_sel, pp, rec.ctypes.data_as(C.c_void_p) if want_records else None, len(rec),
                                                        _p(first, C.c_uint64), None if status is None else _p(status, C.c_uint8),
                                                        len(status) if status is not None else 0, d_out, info))
        n = max([int(info[k].n_points) for k in range(n_sel)], default=0)
        return rec[:int(first[n_sel])], first, (None if status is None else status[:n_sel * n].reshape(n_sel, n)), [info[k] for k in range(n_sel)]

    def batch_correspondences_dev(self, hyp=None, n_sel=None, poses=None):
        """the same, the records left in HBM: (device address of the context-owned record buffer -- valid until the next call --,
        first_record, infos)"""
        d = C.c_void_p()
        _, first, _, infos = self.batch_correspondences(hyp, n_sel, poses, want_status=False, cap_points=0, cap_records=0, want_records=False, d_out=C.byref(d))
        return d.value, first, infos

    def batch_correspondence_sums(self, poses, hyp=None):
        """so_icp_batch_correspondence_sums: poses [n_sel, n_poses, 7] (n_poses <= SUMS_MAX_POSES) -> Sums [n_sel][n_poses] as a flat ctypes
        array (entry k, pose j at [k * n_poses + j]) of the selection `hyp` (None: 0 .. n_sel - 1) of the last batch"""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.ndim == 3 and poses.shape[2] == 7
        n_sel, n_poses = poses.shape[:2]
        hyp = None if hyp is None else np.ascontiguousarray(hyp, np.int32)
        assert hyp is None or len(hyp) == n_sel
        out = (Sums * max(1, n_sel * n_poses))()
        self._check(self.L.so_icp_batch_correspondence_sums(self.h, None if hyp is None else _p(hyp, C.c_int32), n_sel, _p(poses, C.c_double), n_poses, out))
        return out

    def prepare_batch_correspondences(self, n_sel, cap_points, cap_records, hyp=None):
        """so_icp_batch_correspondences at the default poses with pre-built arguments and buffers (timed loops): (call, records, first, info)"""
        hyp = None if hyp is None else np.ascontiguousarray(hyp, np.int32)
        rec = np.zeros(int(cap_records), CORRESPONDENCE_DTYPE); first = np.zeros(n_sel + 1, np.uint64); info = (CorrespondenceInfo * max(n_sel, 1))()
        fn, args = self.L.so_icp_batch_correspondences, (self.h, None if hyp is None else _p(hyp, C.c_int32), n_sel, None, rec.ctypes.data_as(C.c_void_p),
                                                         len(rec), _p(first, C.c_uint64), None, 0, None, info)
        return (lambda _hyp=hyp: fn(*args)), rec, first, info

    def prepare_batch_correspondence_sums(self, poses, hyp=None):
        """so_icp_batch_correspondence_sums with pre-built arguments (timed loops): (call, poses array, Sums array)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).copy()
        n_sel, n_poses = poses.shape[:2]
        hyp = None if hyp is None else np.ascontiguousarray(hyp, np.int32)
        out = (Sums * max(1, n_sel * n_poses))()
        fn, args = self.L.so_icp_batch_correspondence_sums, (self.h, None if hyp is None else _p(hyp, C.c_int32), n_sel, poses.ctypes.data_as(_F64P), n_poses, out)
        return (lambda _hyp=hyp: fn(*args)), poses, out

    # ---- the correspondence sets of a run's frames ----
    def keep_sequence_correspondences(self, on):
        """so_icp_keep_sequence_correspondences: register_sequence / localization_sequence calls from here on leave the sets of all their
        frames for sequence_correspondences() / sequence_correspondence_sums(); returns the C code"""
        return self.L.so_icp_keep_sequence_correspondences(self.h, int(bool(on)))

    def sequence_correspondences(self, frames=None, n_sel=None, poses=None, want_status=True, want_records=True, d_out=None):
        """so_icp_sequence_correspondences for the selection `frames` (None: frames 0 .. n_sel - 1) of the last run, entry k evaluated at
        poses[k] (None: each frame's own optimised pose).  -> (records of the whole selection (CORRESPONDENCE_DTYPE), first_record
        [n_sel + 1]: entry k's records are records[first_record[k]:first_record[k + 1]], status bytes of the whole selection or None,
        first_status [n_sel + 1]: entry k's row is status[first_status[k]:first_status[k + 1]], the n_sel CorrespondenceInfo).  A sizing
        call (counts and offsets only) comes first."""
        frames = None if frames is None else np.ascontiguousarray(frames, np.int32)
        n_sel = len(frames) if frames is not None else int(n_sel)
        poses = None if poses is None else np.ascontiguousarray(poses, np.float64).reshape(n_sel, 7)
        fp = None if frames is None else _p(frames, C.c_int32)
        pp = None if poses is None else _p(poses, C.c_double)
        info = (CorrespondenceInfo * max(n_sel, 1))()
        first = np.zeros(n_sel + 1, np.uint64); first_status = np.zeros(n_sel + 1, np.uint64)
        self._check(self.L.so_icp_sequence_correspondences(self.h, fp, n_sel, pp, None, 0, _p(first, C.c_uint64), None, 0, _p(first_status, C.c_uint64), None, info))
        rec = np.zeros(int(first[n_sel]) if want_records else 0, CORRESPONDENCE_DTYPE)
        status = np.zeros(int(first_status[n_sel]), np.uint8) if want_status else None
        self._check(self.L.so_icp_sequence_correspondences(self.h, fp, n_sel, pp, rec.ctypes.data_as(C.c_void_p) if want_records else None, len(rec),
                                                           _p(first, C.c_uint64), None if status is None else _p(status, C.c_uint8),
                                                           len(status) if status is not None else 0, _p(first_status, C.c_uint64), d_out, info))
        return rec, first, status, first_status, [info[k] for k in range(n_sel)]

    def sequence_correspondences_dev(self, frames=None, n_sel=None, poses=None):
        """the same, the records left in HBM: (device address of the context-owned record buffer -- valid until the next call --,
        first_record, infos)"""
        d = C.c_void_p()
        _, first, _, _, infos = self.sequence_correspondences(frames, n_sel, poses, want_status=False, want_records=False, d_out=C.byref(d))
        return d.value, first, infos

    def sequence_correspondence_sums(self, poses, frames=None):
        """so_icp_sequence_correspondence_sums: poses [n_sel, n_poses, 7] (n_poses <= SUMS_MAX_POSES) -> Sums [n_sel][n_poses] as a flat
        ctypes array (entry k, pose j at [k * n_poses + j]) of the selection `frames` (None: 0 .. n_sel - 1) of the last run"""
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.ndim == 3 and poses.shape[2] == 7
        n_sel, n_poses = poses.shape[:2]
        frames = None if frames is None else np.ascontiguousarray(frames, np.int32)
        assert frames is None or len(frames) == n_sel
        out = (Sums * max(1, n_sel * n_poses))()
        self._check(self.L.so_icp_sequence_correspondence_sums(self.h, None if frames is None else _p(frames, C.c_int32), n_sel, _p(poses, C.c_double), n_poses, out))
        return out

    def prepare_sequence_correspondences(self, n_sel, cap_records, want_records=True):
        """so_icp_sequence_correspondences over frames 0 .. n_sel - 1 at the default poses with pre-built arguments and buffers (timed
        loops): (call, records, first, info)"""
        rec = np.zeros(int(cap_records) if want_records else 0, CORRESPONDENCE_DTYPE); first = np.zeros(n_sel + 1, np.uint64)
        info = (CorrespondenceInfo * max(n_sel, 1))(); d = C.c_void_p()
        fn, args = self.L.so_icp_sequence_correspondences, (self.h, None, n_sel, None, rec.ctypes.data_as(C.c_void_p) if want_records else None, len(rec),
                                                            _p(first, C.c_uint64), None, 0, None, C.byref(d), info)
        return (lambda _d=d: fn(*args)), rec, first, info

    def prepare_sequence_correspondence_sums(self, poses):
        """so_icp_sequence_correspondence_sums over frames 0 .. n_sel - 1 with pre-built arguments (timed loops): (call, poses array, Sums array)"""
        poses = np.ascontiguousarray(poses, dtype=np.float64).copy()
        n_sel, n_poses = poses.shape[:2]
        out = (Sums * max(1, n_sel * n_poses))()
        fn, args = self.L.so_icp_sequence_correspondence_sums, (self.h, None, n_sel, poses.ctypes.data_as(_F64P), n_poses, out)
        return (lambda: fn(*args)), poses, out

    def download_bytes(self, d_ptr, nbytes):
        """nbytes from a device address, through so_icp_download_scan (whole 12-byte units; the buffers of this library are padded)"""
        units = (int(nbytes) + 11) // 12
        out = np.zeros(units * 3, np.float32)
        self._check(self.L.so_icp_download_scan(self.h, C.c_void_p(d_ptr), units, _p(out, C.c_float)))
        return out.view(np.uint8)[:int(nbytes)].copy()

    def neighbours(self, n):
        """the five neighbours (canonical map indices) the last k-NN sweep left for every query (so_icp_debug_neighbours)"""
        out = np.zeros((n, 5), np.uint32)
        self._check(self.L.so_icp_debug_neighbours(self.h, _p(out, C.c_uint32), n))
        return out

    def upload_scan(self, scan):
        scan = _f32(scan).reshape(-1, 3); d = C.c_void_p()
        self._check(self.L.so_icp_upload_scan(self.h, _p(scan, C.c_float), len(scan), 12, C.byref(d)))
        return d.value, len(scan)

    def free_scan(self, d_scan):
        self._check(self.L.so_icp_free_scan(self.h, d_scan))

    def register_dev(self, d_scan, n, pose_in, stats=None, pose_out=None):
        """pose_in / pose_out may be preallocated contiguous float64 arrays (no per-call allocation in a timed loop)."""
        if not (isinstance(pose_in, np.ndarray) and pose_in.dtype == np.float64 and pose_in.flags.c_contiguous):
            pose_in = np.ascontiguousarray(pose_in, dtype=np.float64)
        out = pose_out if pose_out is not None else np.zeros(7)
        st = stats if stats is not None else Stats()
        rc = self.L.so_icp_register_dev(self.h, d_scan, n, pose_in.ctypes.data_as(_F64P), out.ctypes.data_as(_F64P), C.byref(st))
        if rc < 0:
            self._check(rc)
        return rc, out, st

    def prepare_register_dev(self, d_scan, n, pose_in, stats, pose_out):
        """A zero-argument callable that performs exactly one so_icp_register_dev call with pre-built ctypes arguments
        (timed loops: no per-call argument conversion in Python).  pose_in / pose_out: contiguous float64 arrays that
        stay alive; returns the C return code."""
        assert pose_in.dtype == np.float64 and pose_in.flags.c_contiguous and pose_out.dtype == np.float64 and pose_out.flags.c_contiguous
        fn, args = self.L.so_icp_register_dev, (self.h, d_scan, n, pose_in.ctypes.data_as(_F64P), pose_out.ctypes.data_as(_F64P), C.byref(stats))
        return lambda: fn(*args)

    def prepare_register_sequence(self, scans, pose0, deltas, on_device=False):
        """so_icp_register_sequence with pre-built arguments.  scans: contiguous float32 (n, 3) host arrays, or (device pointer, n) pairs
        with on_device.  deltas: (count, 7), row 0 unused.  Returns (call, poses_out (count, 7), guesses_out (count, 7), stats array, n_done):
        call() performs the C call and returns its code."""
        count = len(scans)
        ptrs = (C.c_void_p * count)(); ns = (C.c_size_t * count)()
        for k, sc in enumerate(scans):
            if on_device:
                ptrs[k], ns[k] = sc[0], sc[1]
            else:
                assert isinstance(sc, np.ndarray) and sc.dtype == np.float32 and sc.flags.c_contiguous
                ptrs[k], ns[k] = sc.ctypes.data, len(sc)
        pose0 = np.ascontiguousarray(pose0, dtype=np.float64); deltas = np.ascontiguousarray(deltas, dtype=np.float64).reshape(count, 7)
        out = np.zeros((count, 7)); guesses = np.zeros((count, 7)); st = (Stats * count)(); n_done = C.c_int32(0)
        fn, args = self.L.so_icp_register_sequence, (self.h, count, ptrs, ns, 12, 1 if on_device else 0, pose0.ctypes.data_as(_F64P),
                                                     deltas.ctypes.data_as(_F64P), out.ctypes.data_as(_F64P), guesses.ctypes.data_as(_F64P), st, C.byref(n_done))
        keep = (ptrs, ns, pose0, deltas, scans)
        return (lambda: fn(*args)), out, guesses, st, n_done, keep

    def prepare_localization_sequence(self, scans, pose0, deltas, times, on_device=False):
        """so_icp_localization_sequence with pre-built arguments (register + insert per frame, the reference's order).  scans: contiguous
        float32 (n, 3) host arrays, or (device pointer, n) pairs with on_device.  deltas: (count, 7), row 0 unused; times: count stamps.
        Returns (call, poses_out, guesses_out, stats array, n_done, keep-alive): call() performs the C call and returns its code."""
        count = len(scans)
        ptrs = (C.c_void_p * max(count, 1))(); ns = (C.c_size_t * max(count, 1))()
        for k, sc in enumerate(scans):
            if on_device:
                ptrs[k], ns[k] = sc[0], sc[1]
            else:
                assert isinstance(sc, np.ndarray) and sc.dtype == np.float32 and sc.flags.c_contiguous
                ptrs[k], ns[k] = sc.ctypes.data, len(sc)
        pose0 = np.ascontiguousarray(pose0, dtype=np.float64)
        deltas = np.ascontiguousarray(deltas, dtype=np.float64).reshape(count, 7) if count else np.zeros((1, 7))
        times = np.ascontiguousarray(times, dtype=np.float64).reshape(count) if count else np.zeros(1)
        out = np.zeros((count, 7)); guesses = np.zeros((count, 7)); st = (Stats * max(count, 1))(); n_done = C.c_int32(0)
        fn, args = self.L.so_icp_localization_sequence, (self.h, count, ptrs, ns, 12, 1 if on_device else 0, pose0.ctypes.data_as(_F64P),
                                                         deltas.ctypes.data_as(_F64P), times.ctypes.data_as(_F64P), out.ctypes.data_as(_F64P),
                                                         guesses.ctypes.data_as(_F64P), st, C.byref(n_done))
        keep = (ptrs, ns, pose0, deltas, times, scans)
        return (lambda: fn(*args)), out, guesses, st, n_done, keep

    def localization_sequence(self, scans, pose0, deltas, times, on_device=False):
        """so_icp_localization_sequence: `count` so_icp_localization calls in one, each frame registered and then inserted into the map,
        guess_k = pose_out[k-1] o deltas[k].  Returns (rc, poses_out, guesses_out, stats list, n_done); rc < 0 raises."""
        call, out, guesses, st, n_done, _keep = self.prepare_localization_sequence(scans, pose0, deltas, times, on_device)
        rc = call()
        if rc < 0:
            self._check(rc)
        return rc, out, guesses, list(st)[:len(scans)], n_done.value

    def sequence_announce_next(self, scan, delta):
        """so_icp_sequence_announce_next: the scan that will start the NEXT register_sequence call (None withdraws)"""
        if scan is None:
            self._check(self.L.so_icp_sequence_announce_next(self.h, None, 0, None)); return
        assert isinstance(scan, np.ndarray) and scan.dtype == np.float32 and scan.flags.c_contiguous
        d = np.ascontiguousarray(delta, dtype=np.float64)
        self._check(self.L.so_icp_sequence_announce_next(self.h, _p(scan, C.c_float), len(scan), _p(d, C.c_double)))

    def register_sequence(self, scans, pose0, deltas, on_device=False):
        call, out, guesses, st, n_done, _keep = self.prepare_register_sequence(scans, pose0, deltas, on_device)
        rc = call()
        if rc < 0:
            self._check(rc)
        return rc, out, guesses, list(st), n_done.value

    def register_batch(self, scan, poses_in, d_scan=None, n=None):
        """Same scan, many initial poses (so_icp_register_batch).  scan: host array, or None with (d_scan, n) from upload_scan.
        Returns (number of hypotheses that converged normally, rc[B], poses_out[B,7], stats list)."""
        poses_in = np.ascontiguousarray(poses_in, dtype=np.float64).reshape(-1, 7)
        B = len(poses_in)
        out = np.zeros((B, 7)); rcs = np.zeros(B, np.int32); st = (Stats * B)()
        if d_scan is None:
            scan = _f32(scan).reshape(-1, 3)
            ok = self._check(self.L.so_icp_register_batch(self.h, _p(scan, C.c_float), None, len(scan), 12, _p(poses_in, C.c_double), B,
                                                          _p(out, C.c_double), st, _p(rcs, C.c_int32)))
        else:
            ok = self._check(self.L.so_icp_register_batch(self.h, None, d_scan, n, 12, _p(poses_in, C.c_double), B,
                                                          _p(out, C.c_double), st, _p(rcs, C.c_int32)))
        return ok, rcs, out, list(st)

    def localization(self, initialization, T_w_lidar, planar_points, time_laser_odometry):
        scan = _f32(planar_points).reshape(-1, 3); T = np.ascontiguousarray(T_w_lidar, dtype=np.float64)
        out = np.zeros(7); st = Stats()
        rc = self._check(self.L.so_icp_localization(self.h, int(bool(initialization)), _p(T, C.c_double), _p(scan, C.c_float),
                                                    len(scan), 12, float(time_laser_odometry), _p(out, C.c_double), C.byref(st)))
        return rc, out, st

    def localization_records(self, initialization, T_w_lidar, records, time_laser_odometry):
        """so_icp_localization on records: contiguous float32 array (n, w), stride 4 w bytes (the array itself is handed over, so a
        staged copy of it is recognised)"""
        assert isinstance(records, np.ndarray) and records.dtype == np.float32 and records.flags.c_contiguous and records.ndim == 2
        T = np.ascontiguousarray(T_w_lidar, dtype=np.float64); out = np.zeros(7); st = Stats()
        rc = self._check(self.L.so_icp_localization(self.h, int(bool(initialization)), _p(T, C.c_double), _p(records, C.c_float),
                                                    len(records), 4 * records.shape[1], float(time_laser_odometry), _p(out, C.c_double), C.byref(st)))
        return rc, out, st

    def stage_scan_records(self, records):
        """so_icp_stage_scan on records (see localization_records)"""
        assert isinstance(records, np.ndarray) and records.dtype == np.float32 and records.flags.c_contiguous and records.ndim == 2
        self._check(self.L.so_icp_stage_scan(self.h, _p(records, C.c_float), len(records), 4 * records.shape[1]))

    def localization_dev(self, initialization, T_w_lidar, d_scan, n, time_laser_odometry):
        T = np.ascontiguousarray(T_w_lidar, dtype=np.float64); out = np.zeros(7); st = Stats()
        rc = self._check(self.L.so_icp_localization_dev(self.h, int(bool(initialization)), _p(T, C.c_double), d_scan, n,
                                                        float(time_laser_odometry), _p(out, C.c_double), C.byref(st)))
        return rc, out, st

    def download_scan(self, d_scan, n):
        out = np.zeros((n, 3), np.float32)
        self._check(self.L.so_icp_download_scan(self.h, d_scan, n, _p(out, C.c_float)))
        return out

    def prefilter_announce(self, surf_points):
        """so_icp_prefilter_announce: the raw cloud of the NEXT prefilter_scan call starts its way to HBM now (None withdraws)"""
        if surf_points is None:
            self._check(self.L.so_icp_prefilter_announce(self.h, None, 0, 12)); return
        assert isinstance(surf_points, np.ndarray) and surf_points.dtype == np.float32 and surf_points.flags.c_contiguous
        self._check(self.L.so_icp_prefilter_announce(self.h, _p(surf_points, C.c_float), len(surf_points.reshape(-1, 3)), 12))

    def prefilter_scan(self, surf_points, auto_voxel_size, line_res, plane_res):
        """laserMapping::adjustVoxelSize on the device; returns (d_scan, n, PrefilterInfo)."""
        pts = _f32(surf_points).reshape(-1, 3); d = C.c_void_p(); n = C.c_size_t(0); info = PrefilterInfo()
        self._check(self.L.so_icp_prefilter_scan(self.h, _p(pts, C.c_float), len(pts), 12, int(bool(auto_voxel_size)), float(line_res),
                                                 float(plane_res), C.byref(d), C.byref(n), C.byref(info)))
        return d.value, n.value, info

    def prefilter_scan_records(self, records, auto_voxel_size, line_res, plane_res):
        """so_icp_prefilter_scan on records: float32 array (n, w), stride 4 w bytes; returns (d_scan, n, PrefilterInfo)."""
        rec = _f32(records); assert rec.ndim == 2 and rec.shape[1] >= 3
        d = C.c_void_p(); n = C.c_size_t(0); info = PrefilterInfo()
        self._check(self.L.so_icp_prefilter_scan(self.h, _p(rec, C.c_float), len(rec), 4 * rec.shape[1], int(bool(auto_voxel_size)), float(line_res),
                                                 float(plane_res), C.byref(d), C.byref(n), C.byref(info)))
        return d.value, n.value, info

    def prefilter_intensity(self, n_expected):
        """so_icp_prefilter_intensity: the last pre-filter's intensities -> (float32 array, device address or None)"""
        out = np.zeros(max(int(n_expected), 1), np.float32); d = C.c_void_p(); n = C.c_size_t(0)
        self._check(self.L.so_icp_prefilter_intensity(self.h, _p(out, C.c_float), int(n_expected), C.byref(d), C.byref(n)))
        return out[:n.value].copy(), d.value

    def prefilter_scan_dev(self, d_surf, n, stride_bytes, auto_voxel_size, line_res, plane_res):
        """so_icp_prefilter_scan on a cloud resident in HBM (d_surf: device address); returns (d_scan, n, PrefilterInfo)."""
        d = C.c_void_p(); no = C.c_size_t(0); info = PrefilterInfo()
        self._check(self.L.so_icp_prefilter_scan_dev(self.h, C.c_void_p(d_surf), int(n), int(stride_bytes), int(bool(auto_voxel_size)),
                                                     float(line_res), float(plane_res), C.byref(d), C.byref(no), C.byref(info)))
        return d.value, no.value, info

    def _extract_host(self, fn, payload, shape, layout, lidar_start_time, poses, poses_are_imu, T_i_l):
        """a so_icp_extract_features* host entry: fn(ctx, payload, *shape, layout, time, poses..., clouds out, info); shape: (width, height) or
        (n,).  Returns (records uint8 [n, 32], cloud_surface uint8 [n_surface, 32], FeatureInfo)."""
        raw = np.ascontiguousarray(payload, np.uint8).reshape(-1)
        n = math.prod(map(int, shape))
        rec = np.zeros((n, 32), np.uint8)
        surf = np.zeros((max(n, 1), 32), np.uint8)
        out = (rec.ctypes.data_as(C.c_void_p), surf.ctypes.data_as(C.c_void_p))
        info = self._extract(fn, raw.ctypes.data_as(C.c_void_p), shape, layout, lidar_start_time, poses, poses_are_imu, T_i_l, out)
        return rec, surf[:info.n_surface].copy(), info

    def _extract_dev(self, fn, d_payload, shape, layout, lidar_start_time, poses, poses_are_imu, T_i_l):
        """a so_icp_extract_features*_dev entry; returns (d_nodistortion, d_surface, FeatureInfo)"""
        d_rec = C.c_void_p(); d_surf = C.c_void_p()
        info = self._extract(fn, C.c_void_p(d_payload), shape, layout, lidar_start_time, poses, poses_are_imu, T_i_l, (C.byref(d_rec), C.byref(d_surf)))
        return d_rec.value, d_surf.value, info

    def _extract(self, fn, payload, shape, layout, lidar_start_time, poses, poses_are_imu, T_i_l, out):
        poses = np.zeros((0, 8)) if poses is None else np.ascontiguousarray(poses, np.float64).reshape(-1, 8)
        til = None if T_i_l is None else np.ascontiguousarray(T_i_l, np.float64)
        info = FeatureInfo()
        self._check(fn(self.h, payload, *map(int, shape), C.byref(layout), float(lidar_start_time), _p(poses, C.c_double) if len(poses) else None,
                       len(poses), int(bool(poses_are_imu)), None if til is None else _p(til, C.c_double), *out, C.byref(info)))
        return info

    def extract_features(self, payload, width, height, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """featureExtraction's sweep -> LaserFeature clouds on the device.  payload: the PointCloud2 data (uint8); poses: [m, 8]
        (time, position, quaternion x y z w) or None (no de-skew).  Returns (cloud_nodistortion uint8 [n, 32], cloud_surface
        uint8 [n_surface, 32], FeatureInfo)."""
        return self._extract_host(self.L.so_icp_extract_features, payload, (width, height), layout, lidar_start_time, poses, poses_are_imu, T_i_l)

    def extract_features_dev(self, d_payload, width, height, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """the same on a payload resident in HBM; returns (d_nodistortion, d_surface, FeatureInfo): context-owned device buffers,
        valid until the next call"""
        return self._extract_dev(self.L.so_icp_extract_features_dev, d_payload, (width, height), layout, lidar_start_time, poses, poses_are_imu, T_i_l)

    def extract_features_livox(self, points, n_points, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """livoxHandler's sweep -> LaserFeature clouds on the device.  points: the CustomMsg's points as bytes (uint8), n_points of them
        layout.point_step apart (the last one may end with its last field); the rest as extract_features."""
        return self._extract_host(self.L.so_icp_extract_features_livox, points, (n_points,), layout, lidar_start_time, poses, poses_are_imu, T_i_l)

    def extract_features_livox_dev(self, d_points, n_points, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """the same on points resident in HBM (any byte alignment); returns (d_nodistortion, d_surface, FeatureInfo): context-owned
        device buffers, valid until the next extract_features*_dev call"""
        return self._extract_dev(self.L.so_icp_extract_features_livox_dev, d_points, (n_points,), layout, lidar_start_time, poses, poses_are_imu, T_i_l)

    def extract_features_untimed(self, payload, width, height, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """a sweep without per-point time (assignTimeforPointCloud) -> LaserFeature clouds on the device.  payload: the PointCloud2 data
        (uint8), layout: untimed_layout(...); the rest as extract_features.  Returns (cloud_nodistortion uint8 [info.n_points, 32] --
        the records that remain --, cloud_surface uint8 [n_surface, 32], FeatureInfo)."""
        rec, surf, info = self._extract_host(self.L.so_icp_extract_features_untimed, payload, (width, height), layout, lidar_start_time, poses,
                                             poses_are_imu, T_i_l)
        return rec[:info.n_points].copy(), surf, info

    def extract_features_untimed_dev(self, d_payload, width, height, layout, lidar_start_time, poses=None, poses_are_imu=False, T_i_l=None):
        """the same on a payload resident in HBM; returns (d_nodistortion, d_surface, FeatureInfo): context-owned device buffers
        holding info.n_points and info.n_surface records, valid until the next extract_features*_dev call"""
        return self._extract_dev(self.L.so_icp_extract_features_untimed_dev, d_payload, (width, height), layout, lidar_start_time, poses,
                                 poses_are_imu, T_i_l)

    def deskew_scan(self, records, time_off, lidar_start_time, poses, poses_are_imu, T_i_l=None):
        """featureExtraction::removePointDistortion on the device.  records: uint8 [n, stride] (float x y z at 0 4 8, float time
        at time_off); poses: [n_poses, 8] = time, position, quaternion x y z w.  Returns (rewritten records, DeskewInfo)."""
        rec = np.ascontiguousarray(records, np.uint8).copy()
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 8)
        til = None if T_i_l is None else np.ascontiguousarray(T_i_l, np.float64)
        info = DeskewInfo()
        self._check(self.L.so_icp_deskew_scan(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0], rec.shape[1], int(time_off),
                                              float(lidar_start_time), _p(poses, C.c_double), len(poses), int(bool(poses_are_imu)),
                                              None if til is None else _p(til, C.c_double), C.byref(info)))
        return rec, info

    def transform_cloud(self, records, T_w_lidar):
        """the node's registered scan (pointAssociateToMap over a cloud): records uint8 [n, stride], float x y z at 0 4 8.
        Returns (rewritten records, keep flags [n] uint8, number kept)."""
        rec = np.ascontiguousarray(records, np.uint8).copy()
        T = np.ascontiguousarray(T_w_lidar, np.float64)
        keep = np.zeros(len(rec), np.uint8); nk = C.c_size_t(0)
        self._check(self.L.so_icp_transform_cloud(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0], rec.shape[1], _p(T, C.c_double),
                                                  _p(keep, C.c_uint8), C.byref(nk)))
        return rec, keep, nk.value

    def registered_scan(self, records, T_w_lidar, in_place=False):
        """the node's registered scan as it is published (so_icp_registered_scan): records uint8 [n, stride], float x y z at 0 4 8 ->
        the kept records, transformed, in order: uint8 [n_kept, stride].  in_place: `records` (a contiguous uint8 array) is also the
        output buffer, and the result is a view of its first n_kept records."""
        T = np.ascontiguousarray(T_w_lidar, np.float64)
        if in_place:
            assert isinstance(records, np.ndarray) and records.dtype == np.uint8 and records.ndim == 2 and records.flags.c_contiguous
            rec = out = records
        else:
            rec = np.ascontiguousarray(records, np.uint8)
            out = np.empty_like(rec)
        nk = C.c_size_t(0)
        self._check(self.L.so_icp_registered_scan(self.h, rec.ctypes.data_as(C.c_void_p), rec.shape[0], rec.shape[1], _p(T, C.c_double),
                                                  out.ctypes.data_as(C.c_void_p), C.byref(nk)))
        return out[:nk.value]

    def registered_scan_dev(self, d_records, n, stride, T_w_lidar, want_host=True):
        """the same from records resident in HBM (d_records: device address, e.g. extract_features_dev's d_nodistortion), which stay as
        they are.  Returns (kept records uint8 [n_kept, stride] or None, d_out, n_kept): d_out is a context-owned device buffer
        with the same bytes, valid until the next registered_scan(_dev) call."""
        T = np.ascontiguousarray(T_w_lidar, np.float64)
        out = np.empty((int(n), int(stride)), np.uint8) if want_host else None
        d = C.c_void_p(); nk = C.c_size_t(0)
        self._check(self.L.so_icp_registered_scan_dev(self.h, C.c_void_p(d_records), int(n), int(stride), _p(T, C.c_double),
                                                      None if out is None else out.ctypes.data_as(C.c_void_p), C.byref(d), C.byref(nk)))
        return (None if out is None else out[:nk.value]), d.value, nk.value

    def deskew_scan_dev(self, d_records, n, stride, time_off, lidar_start_time, poses, poses_are_imu, T_i_l=None):
        """the same on records resident in HBM (d_records: device address), rewritten there; returns DeskewInfo"""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 8)
        til = None if T_i_l is None else np.ascontiguousarray(T_i_l, np.float64)
        info = DeskewInfo()
        self._check(self.L.so_icp_deskew_scan_dev(self.h, C.c_void_p(d_records), int(n), int(stride), int(time_off), float(lidar_start_time),
                                                  _p(poses, C.c_double), len(poses), int(bool(poses_are_imu)),
                                                  None if til is None else _p(til, C.c_double), C.byref(info)))
        return info

    # ---- multi-GPU ----
    def comm_init(self, uid_bytes):
        uid = np.frombuffer(bytes(uid_bytes), dtype=np.uint8).copy()
        self._check(self.L.so_icp_comm_init(self.h, _p(uid, C.c_uint8)))

    def comm_init_inprocess(self, group_key):
        self._check(self.L.so_icp_comm_init_inprocess(self.h, int(group_key)))

    def peer_export(self):
        h = np.zeros(PEER_HANDLE_BYTES, np.uint8)
        self._check(self.L.so_icp_peer_export(self.h, _p(h, C.c_uint8)))
        return h.tobytes()

    def peer_connect(self, handles):
        """handles: list of world_size byte strings in rank order; returns the self-test result (bool)."""
        buf = np.frombuffer(b"".join(bytes(h) for h in handles), dtype=np.uint8).copy()
        ok = C.c_int32(0)
        self._check(self.L.so_icp_peer_connect(self.h, _p(buf, C.c_uint8), C.byref(ok)))
        return bool(ok.value)

    def peer_enable(self, on):
        self._check(self.L.so_icp_peer_enable(self.h, int(bool(on))))

    # ---- measurement ----
    def timing(self):
        t = Timing(); self._check(self.L.so_icp_get_timing(self.h, C.byref(t))); return t

    def last_error(self):
        """Text of the context's last error or notice (so_icp_last_error)."""
        return self.L.so_icp_last_error(self.h).decode()

    def reset_timing(self):
        self._check(self.L.so_icp_reset_timing(self.h))

    def set_time_kernels(self, mode):
        self._check(self.L.so_icp_set_time_kernels(self.h, int(mode)))

    def debug_stamps(self):
        out = np.zeros(16, np.uint64)
        self._check(self.L.so_icp_debug_stamps(self.h, _p(out, C.c_uint64)))
        return out

    def debug_knn_stamps(self):
        """(2, workgroups, 16) uint64 records of the k-NN kernel phases (SOICP_ABLATE=128), or None."""
        n = C.c_size_t(0)
        self._check(self.L.so_icp_debug_knn_stamps(self.h, None, 0, C.byref(n)))
        if n.value == 0:
            return None
        out = np.zeros(n.value, np.uint64)
        self._check(self.L.so_icp_debug_knn_stamps(self.h, _p(out, C.c_uint64), n.value, C.byref(n)))
        return out.reshape(2, -1, 16)

    def debug_lm_script(self, form, x0, entries, lm_max=4, max_outer=5, outer_iter=0, want=0):
        """so_icp_debug_lm_script: entries = [(Sums, new_solve), ...] -> (LmScriptStep array, LmScriptResult)."""
        x0 = np.ascontiguousarray(x0, dtype=np.float64); n = len(entries)
        ent = (LmScriptEntry * n)()
        for i, (sums, new_solve) in enumerate(entries):
            ent[i].sums = sums; ent[i].new_solve = int(bool(new_solve))
        steps = (LmScriptStep * n)(); res = LmScriptResult()
        self._check(self.L.so_icp_debug_lm_script(self.h, int(form), _p(x0, C.c_double), int(lm_max), int(max_outer), int(outer_iter), ent, n,
                                                  int(want), steps, C.byref(res)))
        return steps, res

    def synchronize(self):
        self._check(self.L.so_icp_synchronize(self.h))


def registration_error(stats):
    """EstimateRegistrationError (LS.cpp:854-889) from the final normal equations; None when J^T J is singular."""
    out = RegistrationError()
    rc = load().so_icp_registration_error(C.byref(stats), C.byref(out))
    return out if rc == 0 else None


def device_count():
    return int(load().so_icp_device_count())


def comm_unique_id():
    uid = np.zeros(UID_BYTES, np.uint8)
    rc = load().so_icp_comm_unique_id(_p(uid, C.c_uint8))
    if rc:
        raise SoIcpError(f"so_icp_comm_unique_id: {load().so_icp_last_error(None).decode()}")
    return uid.tobytes()


def cells_per_cube(plane_res):
    cell = C.c_double()
    nc = load().so_icp_cells_per_cube(float(plane_res), C.byref(cell))
    return nc, cell.value


def shard_histogram(scan, pose, origin, plane_res, world_size):
    """Queries of `scan` (sensor frame) that fall to each rank under `pose` (so_icp_shard_histogram)."""
    scan = _f32(scan).reshape(-1, 3); pose = np.ascontiguousarray(pose, dtype=np.float64); o = np.ascontiguousarray(origin, dtype=np.int32)
    out = np.zeros(int(world_size), np.int64)
    rc = load().so_icp_shard_histogram(_p(scan, C.c_float), len(scan), 12, _p(pose, C.c_double), _p(o, C.c_int32), float(plane_res), int(world_size),
                                       _p(out, C.c_int64))
    if rc:
        raise SoIcpError(f"so_icp_shard_histogram: {rc}")
    return out


def shard_owner_of_point(p, origin, plane_res, world_size):
    p = _f32(p); o = np.ascontiguousarray(origin, dtype=np.int32)
    return load().so_icp_shard_owner_of_point(_p(p, C.c_float), _p(o, C.c_int32), float(plane_res), int(world_size))


class LmDriver:
    """so_icp_lm_* state machine (Ceres restatement) driven from Python -- used by CPU tests."""

    def __init__(self):
        self.L = load(); self.s = LmState()

    @staticmethod
    def sums(cost, count, Jtr, JtJ_full, hist=None):
        s = Sums(); s.cost = cost; s.count = count
        for i in range(6):
            s.Jtr[i] = Jtr[i]
        k = 0
        for i in range(6):
            for j in range(i, 6):
                s.JtJ[k] = JtJ_full[i][j]; k += 1
        if hist is not None:
            for i in range(16):
                s.hist[i] = hist[i]
        return s

    def begin(self, x0, sums, max_iterations=4):
        x0 = np.ascontiguousarray(x0, dtype=np.float64); nxt = np.zeros(7)
        more = self.L.so_icp_lm_begin(C.byref(self.s), _p(x0, C.c_double), C.byref(sums), max_iterations, _p(nxt, C.c_double))
        return more, nxt

    def feed(self, sums):
        nxt = np.zeros(7)
        more = self.L.so_icp_lm_feed(C.byref(self.s), C.byref(sums), _p(nxt, C.c_double))
        return more, nxt

    def result(self):
        pose = np.zeros(7); st = IterStats()
        self.L.so_icp_lm_result(C.byref(self.s), _p(pose, C.c_double), C.byref(st))
        return pose, st
