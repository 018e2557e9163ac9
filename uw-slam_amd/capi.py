"""ctypes binding of libuwt_hip.so (the C ABI in include/uwt.h).  Plumbing only: every call lands in the HIP
library; there is no Python or CPU implementation of the path here.  Import fails loudly when the shared
library has not been built (run `python -c "import __graft_entry__ as g; g.build()"`).
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libuwt_hip.so")

OK, ERR_INVALID_ARG, ERR_NO_VALID_POINTS, ERR_HIP, ERR_NO_DEVICE, ERR_CAPACITY, ERR_PAIR_FAILED = range(7)
PLANE_IMAGE, PLANE_DEPTH, PLANE_GRADX, PLANE_GRADY = range(4)
MAX_LEVELS = 8
# the domain of the dense warp (include/uwt.h "the dense warp's division"): a seed's |tx|, |ty|, |tz| at most TRANSLATION_MAX or the pair
# fails with ERR_INVALID_ARG; with depth, |depth_scale| * 32767 <= DEPTH_MAX and |depth_scale| / 2^(n_levels - 1) >= DEPTH_MIN or
# uwt_create refuses the context
TRANSLATION_MAX, DEPTH_MAX, DEPTH_MIN = 2.0 ** 125, 2.0 ** 100, 2.0 ** -100
ARITH_OPENCV, ARITH_LEGACY = 0, 1   # uwt_params.arith (include/uwt.h: enum uwt_arith)
NORM_L2, NORM_HAMMING = 0, 1        # enum uwt_norm
MATCH_MAX_ROWS, MATCH_MAX_ROW_BYTES = 4096, 512
KNN2 = np.dtype([("idx0", "<i4"), ("idx1", "<i4"), ("d0", "<f4"), ("d1", "<f4")])           # uwt_knn2
MATCH = np.dtype([("query_idx", "<i4"), ("train_idx", "<i4"), ("distance", "<f4")])          # uwt_match
RANSAC_MAX_HYPOTHESES = 65536
RANSAC_INFO = np.dtype([("status", "<i4"), ("n_inliers", "<i4"), ("best_hypothesis", "<i4"), ("hypotheses_run", "<i4"),
                        ("F", "<f8", (9,))])                                                 # uwt_ransac_info
UWT_MATCH_MAX_ROWS = 4096   # descriptors / key points per set at most (include/uwt.h)
KEYPOINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("response", "<f4"), ("dir_x", "<f4"), ("dir_y", "<f4"),
                     ("octave", "<i4"), ("laplacian", "<i4")])                                  # uwt_keypoint
STATS = np.dtype([("status", "<i4"), ("iterations", "<i4"), ("n_valid", "<i4"), ("error", "<f4")])   # uwt_stats
TRACKING_INFO = np.dtype([("status", "<i4"), ("used_provided", "<i4"), ("n_kp_prev", "<i4"), ("n_kp_cur", "<i4"), ("n_symmetric", "<i4"),
                          ("n_matches", "<i4"), ("best_hypothesis", "<i4"), ("hypotheses_run", "<i4")])   # uwt_tracking_info
WARP_QUALITY = np.dtype([("status", "<i4"), ("n_points", "<i4"), ("n_landed", "<i4"), ("n_covered", "<i4"), ("sum_abs", "<i8"),
                         ("sum_sq", "<i8"), ("sum_abs_unaligned", "<i8"), ("reserved", "<i8")])   # uwt_warp_quality
CLOUD_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("tag", "<u4")])   # uwt_cloud_point
CLOUD_INFO = np.dtype([("status", "<i4"), ("n_rows", "<i4"), ("n_selected", "<i4"), ("n_points", "<i4"), ("offset", "<i8"),
                       ("written", "<i8")])   # uwt_cloud_info
SWEEP_INFO = np.dtype([("status", "<i4"), ("n_selected", "<i4"), ("n_outcome", "<i4", (8,)), ("sum_cost", "<i8"), ("sum_code", "<i8"),
                       ("reserved", "<i8")])   # uwt_sweep_info
# enum uwt_sweep_outcome
SWEEP_NOT_SELECTED, SWEEP_ESTIMATED, SWEEP_BORDER, SWEEP_FEW, SWEEP_LOW_PARALLAX, SWEEP_EDGE, SWEEP_POOR, SWEEP_AMBIGUOUS = range(8)


class Params(C.Structure):
    _fields_ = [
        ("width", C.c_int32), ("height", C.c_int32),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("n_levels", C.c_int32), ("first_level", C.c_int32), ("last_level", C.c_int32), ("max_iters", C.c_int32),
        ("epsilon", C.c_float), ("gain", C.c_float), ("z_factor", C.c_float), ("angle_factor", C.c_float),
        ("depth_scale", C.c_float), ("initial_error", C.c_float),
        ("early_exit", C.c_int32), ("has_depth", C.c_int32), ("handoff_scale_t", C.c_int32),
        ("accumulate_f64", C.c_int32), ("sampler", C.c_int32), ("weights", C.c_int32), ("max_frames", C.c_int32), ("max_pairs", C.c_int32), ("device", C.c_int32),
        ("arith", C.c_int32),
    ]


class Tuning(C.Structure):
    """uwt_tuning: launch-shape switches of a context (never what is computed)."""
    _fields_ = [
        ("split", C.c_int32), ("split_min", C.c_int32), ("split_min_px", C.c_int64), ("stream_bytes", C.c_int64),
        ("tail_update", C.c_int32), ("target_blocks", C.c_int32), ("coarse", C.c_int32), ("coarse_batch_px", C.c_int32),
        ("coarse_weighted", C.c_int32), ("overlap_gradients", C.c_int32), ("first_poll", C.c_int32), ("chained", C.c_int32),
        ("speculation", C.c_int32), ("fused_stages", C.c_int32), ("pyramid_batch", C.c_int32), ("typed_loads", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


class RansacParams(C.Structure):
    """uwt_ransac_params: distance_ / confidence_ of RobustMatcher (include/Tracker.h:82-83), the hypothesis budget, the seed"""
    _fields_ = [("distance", C.c_double), ("confidence", C.c_double), ("max_hypotheses", C.c_int32), ("seed", C.c_uint32)]


class SurfParams(C.Structure):
    """uwt_surf_params: SURF_CUDA's hessianThreshold, nOctaves, nOctaveLayers, upright"""
    _fields_ = [("hessian_threshold", C.c_double), ("n_octaves", C.c_int32), ("n_octave_layers", C.c_int32), ("upright", C.c_int32)]


class OrbParams(C.Structure):
    """uwt_orb_params: cuda::ORB::create()'s nfeatures, nlevels, edgeThreshold, fastThreshold, and upright"""
    _fields_ = [("n_features", C.c_int32), ("n_levels", C.c_int32), ("edge_threshold", C.c_int32), ("fast_threshold", C.c_int32),
                ("upright", C.c_int32)]


class TrackingParams(C.Structure):
    """uwt_tracking_params: the SURF and RANSAC parameters, ratio_ and the `n_matches_ < 110` rule of System::Tracking"""
    _fields_ = [("surf", SurfParams), ("ransac", RansacParams), ("ratio", C.c_float), ("min_matches", C.c_int32)]


class TrackingOrbParams(C.Structure):
    """uwt_tracking_orb_params: the same record for RobustMatcher(1), with the ORB parameters in SURF's place (56 bytes)"""
    _fields_ = [("orb", OrbParams), ("ransac", RansacParams), ("ratio", C.c_float), ("min_matches", C.c_int32)]


class TrackingIO(C.Structure):
    """uwt_tracking_io: device pointers of one uwt_tracking_batch_async call"""
    _fields_ = [("d_prev_kp", C.c_void_p), ("d_n_prev", C.c_void_p), ("d_poses", C.c_void_p), ("d_stats", C.c_void_p),
                ("d_info", C.c_void_p), ("d_good", C.c_void_p), ("d_kept_prev", C.c_void_p), ("d_kept_cur", C.c_void_p),
                ("d_n_matches", C.c_void_p)]


class WarpImageIO(C.Structure):
    """uwt_warp_image_io: device pointers of one uwt_warp_image_batch_async call"""
    _fields_ = [("d_warped", C.c_void_p), ("d_valid", C.c_void_p), ("d_absdiff", C.c_void_p), ("d_quality", C.c_void_p)]


class CloudParams(C.Structure):
    """uwt_cloud_params: mode (0 the reference's visualiser, 1 world), stride, skip_invalid, source (0 dense, 1 candidates), threshold"""
    _fields_ = [("mode", C.c_int32), ("stride", C.c_int32), ("skip_invalid", C.c_int32), ("source", C.c_int32), ("threshold", C.c_double),
                ("reserved", C.c_int32 * 2)]


def default_cloud_params(**over):
    """uwt_default_cloud_params: {0, 100, 0, 0, 20.0}, the reference's call; keyword arguments override fields"""
    return _defaults(CloudParams(), "uwt_default_cloud_params", over)


class SweepParams(C.Structure):
    """uwt_sweep_params: the level, the pixel source and its threshold, views, hypotheses, patch radius and the decision's constants"""
    _fields_ = [("lvl", C.c_int32), ("source", C.c_int32), ("threshold", C.c_double), ("n_views", C.c_int32), ("n_hyp", C.c_int32),
                ("radius", C.c_int32), ("max_mean_abs", C.c_int32), ("uniq_num", C.c_int32), ("uniq_den", C.c_int32),
                ("min_parallax", C.c_int32), ("refine", C.c_int32), ("reserved", C.c_int32 * 4)]


class SweepIO(C.Structure):
    """uwt_sweep_io: device pointers of one uwt_sweep_depth_batch_async call"""
    _fields_ = [("d_depth", C.c_void_p), ("d_cost", C.c_void_p), ("d_outcome", C.c_void_p), ("d_info", C.c_void_p)]


def default_sweep_params(**over):
    """uwt_default_sweep_params: {0, 1, 20.0, 1, 32, 2, 12, 3, 4, 4, 1}; keyword arguments override fields"""
    return _defaults(SweepParams(), "uwt_default_sweep_params", over)


def sweep_hypotheses(z_near, z_far, depth_scale, n):
    """uwt_sweep_hypotheses: n u16 depth codes uniform in inverse depth from z_near to z_far (a host helper, no context)"""
    codes = np.zeros(max(int(n), 1), np.uint16)
    st = lib().uwt_sweep_hypotheses(z_near, z_far, depth_scale, int(n), _p(codes, C.c_uint16))
    if st:
        raise UwtError(st, "uwt_sweep_hypotheses: codes not strictly increasing, outside 1..32767, or an argument out of range")
    return codes[:n]


class TableOptions(C.Structure):
    """uwt_table_options: the weights (0 identity, 1 Tukey, 2 Huber) and sampler (0 round(), 1 bilinear) of one batched table call"""
    _fields_ = [("weights", C.c_int32), ("sampler", C.c_int32), ("reserved", C.c_int32 * 6)]


class SeedOptions(C.Structure):
    """uwt_seed_options: how a seeded call's pose crosses the level boundaries (handoff 0 the reference's hand-off, 1 keep)"""
    _fields_ = [("handoff", C.c_int32), ("reserved", C.c_int32 * 7)]


HANDOFF_REFERENCE, HANDOFF_KEEP = 0, 1


class Level(C.Structure):
    _fields_ = [("w", C.c_int32), ("h", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("img_w", C.c_int32), ("img_h", C.c_int32), ("pitch", C.c_int32)]   # w, h: point grid; img_*: the level's image


class Stats(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("n_valid", C.c_int32), ("error", C.c_float)]


class Accum(C.Structure):
    _fields_ = [("A", C.c_double * 21), ("jtr", C.c_double * 6), ("sum_r2", C.c_int64),
                ("n_valid", C.c_int32), ("pad", C.c_int32)]


class PairState(C.Structure):
    """uwt_pair_state: a pair's state inside an alignment (uwt_gn_update_records)"""
    _fields_ = [("pose", C.c_float * 7), ("last_error", C.c_float), ("error", C.c_float), ("level_done", C.c_int32),
                ("status", C.c_int32), ("iters", C.c_int32), ("n_valid", C.c_int32)]


# the same record as a numpy dtype: arrays of states go in and out of Context.gn_update_records
PAIR_STATE_DTYPE = np.dtype([("pose", "<f4", (7,)), ("last_error", "<f4"), ("error", "<f4"), ("level_done", "<i4"), ("status", "<i4"),
                             ("iters", "<i4"), ("n_valid", "<i4")])


JACOBIAN_REFERENCE, JACOBIAN_METRIC = 0, 1   # enum uwt_jacobian

ABI_VERSION = 4   # UWT_ABI_VERSION of the include/uwt.h this table was written from
# The prototype of every entry include/uwt.h declares, in the header's order: name -> (return type, argument types).  lib() sets them
# on the library, so a call site passes plain Python values and ctypes converts each to the width the C side reads.  Every pointer
# or array parameter is P (it takes None, an address as an int, byref(x), a ctypes array or pointer); a scalar has its exact type.
# tests/test_abi_cpu.py compares the table with the header, declaration by declaration.
ci, cs, i32, i64, f32, f64, sz, P = C.c_int, C.c_char_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t, C.c_void_p
PROTOTYPES = {
    "uwt_default_params": (ci, (P, i32, i32, f32, f32, f32, f32)),
    "uwt_create": (ci, (P, P)),
    "uwt_update_params": (ci, (P, P)),
    "uwt_get_params": (ci, (P, P)),
    "uwt_get_tuning": (ci, (P, P)),
    "uwt_set_tuning": (ci, (P, P)),
    "uwt_destroy": (ci, (P,)),
    "uwt_level_info": (ci, (P, i32, P)),
    "uwt_status_string": (cs, (ci,)),
    "uwt_last_error": (cs, (P,)),
    "uwt_abi_version": (ci, ()),
    "uwt_source_id": (cs, ()),
    "uwt_set_frame": (ci, (P, i32, P, sz, P, sz)),
    "uwt_upload_frames": (ci, (P, i32, i32, P, P)),
    "uwt_upload_frames_async": (ci, (P, i32, i32, P, P)),
    "uwt_host_alloc": (ci, (sz, P)),
    "uwt_host_free": (ci, (P,)),
    "uwt_plane_device_ptr": (ci, (P, i32, i32, i32, P)),
    "uwt_get_plane": (ci, (P, i32, i32, i32, P)),
    "uwt_build_pyramids": (ci, (P, i32, i32)),
    "uwt_apply_gradient": (ci, (P, i32, i32)),
    "uwt_estimate_pose_batch": (ci, (P, i32, P, P, P, P)),
    "uwt_track_batch_async": (ci, (P, i32, i32, i32, i32, P, P, P, P)),
    "uwt_track_batch_host_async": (ci, (P, i32, i32, i32, i32, P, P, P, P, P)),
    "uwt_wait_ticket": (ci, (P, i64)),
    "uwt_sync": (ci, (P,)),
    "uwt_set_deferred": (ci, (P, i32)),
    "uwt_stream": (ci, (P, P)),
    "uwt_profile_enable": (ci, (P, i32)),
    "uwt_profile_read": (ci, (P, P, P, P)),
    "uwt_profile_read_levels": (ci, (P, P, P, i32)),
    "uwt_profile_clock": (ci, (P, P)),
    "uwt_halve_u8": (ci, (P, P, i32, i32, P)),
    "uwt_halve_u16": (ci, (P, P, i32, i32, P)),
    "uwt_half_size": (ci, (i32,)),
    "uwt_resize_half_u8": (ci, (P, P, i32, i32, P)),
    "uwt_resize_half_u16": (ci, (P, P, i32, i32, P)),
    "uwt_scharr3": (ci, (P, P, i32, i32, P, P)),
    "uwt_warp": (ci, (P, i32, P, i32, P, P)),
    "uwt_residual_jacobian": (ci, (P, i32, i32, i32, P, P, P, P, P)),
    "uwt_residual_jacobian_weighted": (ci, (P, i32, i32, i32, P, P, P, P, P, P, P, P)),
    "uwt_ls_accumulate": (ci, (P, P, P, P, i32, i32, P, P, P, P)),
    "uwt_ls_accumulate_sse": (ci, (P, P, P, P, i32, i32, i32, P, P, P, P)),
    "uwt_se3_exp": (ci, (P, P, P)),
    "uwt_se3_mul": (ci, (P, P, P, P)),
    "uwt_se3_matrix": (ci, (P, P, P)),
    "uwt_se3_handoff": (ci, (P, P, i32)),
    "uwt_solve_delta": (ci, (P, P, P, P, P, P)),
    "uwt_gn_update_records": (ci, (P, i32, i32, i32, i32, i32, P, P, i32, i32, i32, f32, f32, i32, P, P, P)),
    "uwt_estimate_pose_points": (ci, (P, i32, i32, P, P, P, P)),
    "uwt_robust_weights": (ci, (P, P, i32, i32, P, P, P)),
    "uwt_gradient_magnitude": (ci, (P, i32, i32, P)),
    "uwt_obtain_candidate_points": (ci, (P, i32, i32, f64, P, i32, P)),
    "uwt_obtain_candidate_points_batch": (ci, (P, i32, i32, i32, f64, P, i32, P)),
    "uwt_obtain_patch_points": (ci, (P, i32, P, i32, P, i32, P)),
    "uwt_add_patch_points": (ci, (P, i32, P, i32, i32, P, i32, P)),
    "uwt_obtain_patch_points_batch": (ci, (P, i32, P, P, P, P, i32, P)),
    "uwt_track_features_batch_async": (ci, (P, i32, P, P, P, P, P, P)),
    "uwt_estimate_pose_features_batch": (ci, (P, i32, P, P, P, P, P, P)),
    "uwt_default_table_options": (ci, (P,)),
    "uwt_track_features_batch_opt_async": (ci, (P, i32, P, P, P, P, P, P, P)),
    "uwt_estimate_pose_features_batch_opt": (ci, (P, i32, P, P, P, P, P, P, P)),
    "uwt_track_candidates_batch_async": (ci, (P, i32, P, P, f64, P, P)),
    "uwt_estimate_pose_candidates_batch": (ci, (P, i32, P, P, f64, P, P)),
    "uwt_track_candidates_batch_opt_async": (ci, (P, i32, P, P, f64, P, P, P)),
    "uwt_estimate_pose_candidates_batch_opt": (ci, (P, i32, P, P, f64, P, P, P)),
    "uwt_knn_match_batch": (ci, (P, i32, i32, i32, P, P, P, P, i32, P)),
    "uwt_match_descriptors_batch": (ci, (P, i32, i32, i32, P, P, P, P, i32, f32, P, P)),
    "uwt_match_descriptors_batch_async": (ci, (P, i32, i32, i32, P, P, P, P, i32, f32, P, P)),
    "uwt_default_ransac_params": (ci, (P,)),
    "uwt_ransac_iterations": (i32, (f64, i32, i32, i32)),
    "uwt_ransac_inliers_batch": (ci, (P, i32, P, P, i32, P, P, P, P, i32, P, P, P, P, P)),
    "uwt_ransac_inliers_batch_async": (ci, (P, i32, P, P, i32, P, P, P, P, i32, P, P, P, P, P)),
    "uwt_default_surf_params": (ci, (P,)),
    "uwt_keypoint_angle_deg": (f64, (f32, f32)),
    "uwt_surf_detect_describe_batch": (ci, (P, i32, P, P, i32, P, P, P)),
    "uwt_surf_detect_describe_batch_async": (ci, (P, i32, P, P, i32, P, P, P)),
    "uwt_surf_describe_batch": (ci, (P, i32, P, P, P, P, i32, P, P)),
    "uwt_surf_integral": (ci, (P, i32, P)),
    "uwt_surf_response_layer": (ci, (P, i32, i32, i32, P, P, P)),
    "uwt_default_orb_params": (ci, (P,)),
    "uwt_orb_level_quota": (ci, (i32, i32, P)),
    "uwt_orb_default_pattern": (ci, (P,)),
    "uwt_orb_layer_size": (ci, (i32, i32, i32, P, P)),
    "uwt_orb_set_pattern": (ci, (P, P)),
    "uwt_orb_detect_describe_batch": (ci, (P, i32, P, P, i32, P, P, P)),
    "uwt_orb_detect_describe_batch_async": (ci, (P, i32, P, P, i32, P, P, P)),
    "uwt_orb_describe_batch": (ci, (P, i32, P, P, P, P, i32, P, P)),
    "uwt_orb_layer": (ci, (P, i32, i32, P, P, P)),
    "uwt_orb_fast_scores": (ci, (P, i32, i32, P)),
    "uwt_orb_harris": (ci, (P, i32, i32, P, i32, P)),
    "uwt_default_tracking_params": (ci, (P,)),
    "uwt_tracking_batch_async": (ci, (P, i32, P, P, P, i32, P)),
    "uwt_tracking_batch": (ci, (P, i32, P, P, P, i32, P, P, P, P, P, P, P, P)),
    "uwt_default_tracking_orb_params": (ci, (P,)),
    "uwt_tracking_orb_batch_async": (ci, (P, i32, P, P, P, i32, P)),
    "uwt_tracking_orb_batch": (ci, (P, i32, P, P, P, i32, P, P, P, P, P, P, P, P)),
    "uwt_match_descriptors_device_async": (ci, (P, i32, i32, i32, P, P, P, P, i32, f32, P, P)),
    "uwt_obtain_image_transformed": (ci, (P, i32, i32, P, P, i32, P, P)),
    "uwt_warp_image_batch_async": (ci, (P, i32, P, P, i32, P, P)),
    "uwt_warp_image_batch": (ci, (P, i32, P, P, i32, P, P, P, P, P)),
    "uwt_warp_mosaic": (ci, (P, i32, i32, i32, P, P)),
    "uwt_default_cloud_params": (ci, (P,)),
    "uwt_point_cloud_batch_async": (ci, (P, i32, P, P, P, P, i64, P)),
    "uwt_point_cloud_batch": (ci, (P, i32, P, P, P, P, i64, P)),
    "uwt_point_cloud_points": (ci, (P, i32, P, i32, P, P, P, i64, P)),
    "uwt_ingest_create": (ci, (P, P, i32, i32, i32, i32, i32, P, P)),
    "uwt_ingest_destroy": (ci, (P,)),
    "uwt_ingest_maps": (ci, (P, P, P)),
    "uwt_ingest_undistort": (ci, (P, P, sz, P)),
    "uwt_ingest_calculate_roi": (ci, (P, P, sz, P)),
    "uwt_ingest_frame": (ci, (P, P, i32, P, sz, i32, i32)),
    "uwt_accumulate_trajectory": (ci, (P, P, i32, P, f32, i32, P)),
    "uwt_accumulate_trajectory_scan": (ci, (P, P, i32, P, f32, i32, P)),
    "uwt_accumulate_trajectory_device_async": (ci, (P, P, i32, P, f32, i32, P)),
    "uwt_accumulate_trajectory_device_from_async": (ci, (P, P, i32, P, f32, i32, P)),
    "uwt_default_seed_options": (ci, (P,)),
    "uwt_estimate_pose_batch_seeded": (ci, (P, i32, P, P, P, P, P, P)),
    "uwt_track_batch_seeded_async": (ci, (P, i32, i32, i32, i32, P, P, P, P, P, P)),
    "uwt_track_features_batch_seeded_async": (ci, (P, i32, P, P, P, P, P, P, P, P, P)),
    "uwt_estimate_pose_features_batch_seeded": (ci, (P, i32, P, P, P, P, P, P, P, P, P)),
    "uwt_track_candidates_batch_seeded_async": (ci, (P, i32, P, P, f64, P, P, P, P, P)),
    "uwt_estimate_pose_candidates_batch_seeded": (ci, (P, i32, P, P, f64, P, P, P, P, P)),
    "uwt_tracking_batch_seeded_async": (ci, (P, i32, P, P, P, i32, P, P, P)),
    "uwt_tracking_orb_batch_seeded_async": (ci, (P, i32, P, P, P, i32, P, P, P)),
    "uwt_tracking_batch_seeded": (ci, (P, i32, P, P, P, i32, P, P, P, P, P, P, P, P, P, P)),
    "uwt_tracking_orb_batch_seeded": (ci, (P, i32, P, P, P, i32, P, P, P, P, P, P, P, P, P, P)),
    "uwt_predict_seeds_device_async": (ci, (P, i32, P, P, P)),
    "uwt_predict_seeds": (ci, (P, i32, P, P, P)),
    "uwt_set_jacobian": (ci, (P, i32)),
    "uwt_get_jacobian": (ci, (P, P)),
    "uwt_default_sweep_params": (ci, (P,)),
    "uwt_sweep_hypotheses": (ci, (f64, f64, f64, i32, P)),
    "uwt_sweep_depth_batch_async": (ci, (P, i32, P, P, P, P, P, P)),
    "uwt_sweep_depth_batch": (ci, (P, i32, P, P, P, P, P, P, P, P, P)),
    "uwt_debug_guards": (ci, (P, i64)),
    "uwt_debug_check_guards": (ci, (P, P)),
    "uwt_debug_window_open": (ci, (P, P)),
}
SYMBOLS = list(PROTOTYPES)   # every symbol include/uwt.h declares (tests check the library exports all of them)

_lib = None


class UwtError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__("uwt status %d: %s" % (status, msg))
        self.status = status


def _share_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  If libuwt_hip.so pulled in the
    system copy first, a later `import torch` would load a second HIP runtime into the process (two device states,
    "No HIP GPUs are available", unordered streams).  Loading torch's copy first makes both use one runtime; without
    torch installed the system runtime is used."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec and spec.origin:
            cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
            if os.path.exists(cand):
                C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass


def lib():
    """Loads libuwt_hip.so and sets PROTOTYPES on it; raises if it is missing (no fallback) or was built from another ABI version."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libuwt_hip.so not built at %s — run __graft_entry__.build()" % LIB_PATH)
        _share_torch_hip_runtime()
        loaded = C.CDLL(LIB_PATH)
        stale = [name for name in PROTOTYPES if not hasattr(loaded, name)]
        version = None if stale else loaded.uwt_abi_version()
        if version != ABI_VERSION:
            raise ImportError("libuwt_hip.so at %s is stale (%s; this binding is written for ABI version %d) — rebuild it: run "
                              "__graft_entry__.build()" % (LIB_PATH, "no " + stale[0] if stale else "ABI version %d" % version, ABI_VERSION))
        for name, (restype, argtypes) in PROTOTYPES.items():
            fn = getattr(loaded, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = loaded
    return _lib


def source_id():
    """uwt_source_id(): sha256 of the sources and flags the loaded library was built from"""
    return lib().uwt_source_id().decode()


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _ref(rec):
    """byref of an optional record: None stays None (NULL, the entry's defaults)"""
    return None if rec is None else C.byref(rec)


DEFAULT_ARITH = None   # None: the library's default (ARITH_OPENCV); the parity suite sets it to run every test under both sets


def _set_fields(rec, over):
    for k, v in over.items():
        if not hasattr(rec, k):
            raise AttributeError(k)
        setattr(rec, k, v)


def _defaults(rec, entry, over=None, *args):
    """rec as the library's uwt_default_* entry fills it (args: what the entry takes besides the record), then the fields in over set"""
    st = getattr(lib(), entry)(C.byref(rec), *args)
    if st:
        raise UwtError(st, entry)
    _set_fields(rec, over or {})
    return rec


def default_params(width, height, fx, fy, cx, cy, **over):
    if DEFAULT_ARITH is not None:
        over = {"arith": DEFAULT_ARITH, **over}
    return _defaults(Params(), "uwt_default_params", over, width, height, fx, fy, cx, cy)


def table_options(weights=None, sampler=None):
    """uwt_default_table_options ({0, 0}) with the given fields set"""
    o = _defaults(TableOptions(), "uwt_default_table_options")
    if weights is not None:
        o.weights = weights
    if sampler is not None:
        o.sampler = sampler
    return o


def seed_options(handoff=None):
    """uwt_default_seed_options ({0}) with the hand-off set (HANDOFF_REFERENCE / HANDOFF_KEEP, or "reference" / "keep")"""
    o = _defaults(SeedOptions(), "uwt_default_seed_options")
    if handoff is not None:
        o.handoff = {"reference": HANDOFF_REFERENCE, "keep": HANDOFF_KEEP}.get(handoff, handoff)
    return o


def _host_seeds(seeds, n):
    """Host seeds as the synchronous seeded calls take them: None, or n x 7 float32 (a row with a non-finite entry or a translation entry
    above TRANSLATION_MAX in magnitude is refused by the device, for its pair alone)"""
    if seeds is None:
        return None, None
    a = np.ascontiguousarray(seeds, np.float32).reshape(-1, 7)
    if a.shape[0] != n:
        raise ValueError("seeds: %d rows for %d pairs" % (a.shape[0], n))
    return a, _p(a, C.c_float)


def _sopt(handoff):
    if isinstance(handoff, SeedOptions):
        return C.byref(handoff)
    return None if handoff is None else C.byref(seed_options(handoff))


def _pair_lists(ref_slots, tgt_slots):
    """The reference and the target slots of a batch call as flat int32 arrays"""
    return np.ascontiguousarray(ref_slots, np.int32).reshape(-1), np.ascontiguousarray(tgt_slots, np.int32).reshape(-1)


def _result_buffers(n):
    """Host room for the results of n pairs, never of size zero: poses [n, 7] float32 and n uwt_stats"""
    return np.empty((max(n, 1), 7), np.float32), (Stats * max(n, 1))()


def _accum_fields(acc):
    """A uwt_accum as the residual calls return it: A the full 6 x 6 matrix of the upper triangle the record holds row by row"""
    A = np.zeros((6, 6))
    A[np.triu_indices(6)] = acc.A   # (0, 0), (0, 1) .. (0, 5), (1, 1) .. (5, 5)
    A += np.triu(A, 1).T
    return dict(A=A, jtr=np.array(acc.jtr), sum_r2=int(acc.sum_r2), n_valid=int(acc.n_valid))


def _stats_list(stats, n):
    return [dict(status=s.status, iterations=s.iterations, n_valid=s.n_valid, error=s.error) for s in stats[:n]]


def default_ransac_params(**over):
    """uwt_default_ransac_params: distance 3.0, confidence 0.99, max_hypotheses 1000, seed 0"""
    return _defaults(RansacParams(), "uwt_default_ransac_params", over)


def default_surf_params(**over):
    """uwt_default_surf_params: hessian_threshold 100, n_octaves 4, n_octave_layers 2, upright 0"""
    return _defaults(SurfParams(), "uwt_default_surf_params", over)


def default_orb_params(**over):
    """uwt_default_orb_params: n_features 500, n_levels 8, edge_threshold 31, fast_threshold 20, upright 0"""
    return _defaults(OrbParams(), "uwt_default_orb_params", over)


def orb_level_quota(n_features, n_levels):
    """uwt_orb_level_quota: the key points each layer of the ORB pyramid may keep, on the host"""
    out = np.zeros(max(n_levels, 1), np.int32)
    st = lib().uwt_orb_level_quota(n_features, n_levels, _p(out, C.c_int32))
    if st:
        raise UwtError(st, "uwt_orb_level_quota")
    return out


def orb_default_pattern():
    """uwt_orb_default_pattern: the default sampling pattern, int8 [256, 4] (x0, y0, x1, y1)"""
    out = np.zeros((256, 4), np.int8)
    st = lib().uwt_orb_default_pattern(_p(out, C.c_int8))
    if st:
        raise UwtError(st, "uwt_orb_default_pattern")
    return out


def orb_layer_size(w, h, level):
    """uwt_orb_layer_size: (w_l, h_l) of a layer of the ORB pyramid"""
    lw, lh = C.c_int32(0), C.c_int32(0)
    st = lib().uwt_orb_layer_size(w, h, level, C.byref(lw), C.byref(lh))
    if st:
        raise UwtError(st, "uwt_orb_layer_size")
    return lw.value, lh.value


def _tracking_params(p, entry, detector, detector_over, ransac, over):
    _defaults(p, entry)
    for rec, d in ((getattr(p, detector), detector_over or {}), (p.ransac, ransac or {}), (p, over)):
        _set_fields(rec, d)
    return p


def default_tracking_params(surf=None, ransac=None, **over):
    """uwt_default_tracking_params: the SURF and RANSAC defaults, ratio 0.65, min_matches 110.  surf / ransac: dicts of fields of the
    nested records to change; the other keywords are fields of the record itself."""
    return _tracking_params(TrackingParams(), "uwt_default_tracking_params", "surf", surf, ransac, over)


def default_tracking_orb_params(orb=None, ransac=None, **over):
    """uwt_default_tracking_orb_params: the ORB and RANSAC defaults, ratio 0.65, min_matches 110; orb / ransac / the other keywords as
    in default_tracking_params."""
    return _tracking_params(TrackingOrbParams(), "uwt_default_tracking_orb_params", "orb", orb, ransac, over)


def keypoint_angle_deg(dir_x, dir_y):
    """uwt_keypoint_angle_deg: cv::KeyPoint::angle of a key point's direction, degrees in [0, 360), on the host"""
    return float(lib().uwt_keypoint_angle_deg(dir_x, dir_y))


def ransac_iterations(confidence, n, inliers, max_hypotheses):
    """uwt_ransac_iterations: need(k) of the RANSAC contract, on the host (no context, no device)"""
    return int(lib().uwt_ransac_iterations(confidence, n, inliers, max_hypotheses))


class _Pinned:
    """Owner of one uwt_host_alloc block; the numpy view below keeps it alive."""

    def __init__(self, nbytes):
        self.ptr = C.c_void_p()
        st = lib().uwt_host_alloc(nbytes,C.byref(self.ptr))
        if st:
            raise UwtError(st, "uwt_host_alloc(%d)" % nbytes)

    def __del__(self):
        try:
            lib().uwt_host_free(self.ptr)
        except Exception:
            pass


class _PinnedArray(np.ndarray):
    """ndarray view that keeps its page-locked block alive (views and slices inherit the reference)."""

    def __new__(cls, arr, owner):
        obj = arr.view(cls)
        obj._owner = owner
        return obj

    def __array_finalize__(self, obj):
        self._owner = getattr(obj, "_owner", None)


def pinned_empty(shape, dtype):
    """Page-locked numpy array (hipHostMalloc through the C ABI) for upload_frames_async."""
    dtype = np.dtype(dtype)
    count = int(np.prod(shape))
    nbytes = max(count * dtype.itemsize, 1)
    owner = _Pinned(nbytes)
    buf = (C.c_uint8 * nbytes).from_address(owner.ptr.value)
    arr = np.frombuffer(buf, dtype=dtype, count=count).reshape(shape)
    return _PinnedArray(arr, owner)


class Context:
    """Owns one uwt_ctx (device buffers + stream) — the state behind a reference `Tracker` instance."""

    def __init__(self, params, tuning=None):
        """tuning: dict of uwt_tuning fields to change from their defaults (launch shapes only; the A/B tools and the tests
        that run one form against another use it).  UwtError(ERR_INVALID_ARG) for parameters uwt_create refuses — with has_depth, a
        depth_scale outside [DEPTH_MIN * 2^(n_levels - 1), DEPTH_MAX / 32767] in magnitude (zero apart) among them."""
        self.params = params
        self._h = C.c_void_p()
        st = lib().uwt_create(C.byref(params), C.byref(self._h))
        if st:
            raise UwtError(st, lib().uwt_status_string(st).decode())
        self.w, self.h = params.width, params.height
        if tuning:
            self.set_tuning(**tuning)

    def get_tuning(self):
        t = Tuning()
        self._chk(lib().uwt_get_tuning(self._h, C.byref(t)))
        return t

    def set_tuning(self, **over):
        """Change launch-shape switches of the live context (uwt_set_tuning)."""
        t = self.get_tuning()
        for k, v in over.items():
            if k == "reserved" or not hasattr(t, k):
                raise AttributeError(k)
            setattr(t, k, int(v))
        self._chk(lib().uwt_set_tuning(self._h, C.byref(t)))

    def get_jacobian(self):
        """The context's Jacobian mode (uwt_get_jacobian): JACOBIAN_REFERENCE or JACOBIAN_METRIC."""
        out = C.c_int32(0)
        self._chk(lib().uwt_get_jacobian(self._h, C.byref(out)))
        return out.value

    def set_jacobian(self, mode):
        """uwt_set_jacobian: 0 / "reference" the reference's Jw (pixel coordinates in columns 2..5; the default), 1 / "metric" the
        3-D point's coordinates.  Applies to every later call that forms a Jacobian; metric is meant to run with handoff "keep"."""
        mode = {"reference": JACOBIAN_REFERENCE, "metric": JACOBIAN_METRIC}.get(mode, mode)
        self._chk(lib().uwt_set_jacobian(self._h, int(mode)))

    def close(self):
        if self._h:
            lib().uwt_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, allow=()):
        if st and st not in allow:
            raise UwtError(st, lib().uwt_last_error(self._h).decode())
        return st

    def _chk_pairs(self, st, raise_on_pair_failure):
        """_chk for a batch call: ERR_PAIR_FAILED (some pair's status says why) passes unless asked to raise"""
        return self._chk(st, allow=() if raise_on_pair_failure else (ERR_PAIR_FAILED,))

    def debug_guards(self, guard_bytes):
        """Test instrumentation (uwt_debug_guards): guard gaps of guard_bytes around and inside every growable scratch block of the
        context from now on; 0 turns them off.  Waits for the context's work and releases the blocks."""
        self._chk(lib().uwt_debug_guards(self._h, int(guard_bytes)))

    def debug_check_guards(self):
        """(damaged bytes, the library's description of the first damaged gap or "") over the gaps of every block's last use
        (uwt_debug_check_guards)"""
        n = C.c_int64(-1)
        self._chk(lib().uwt_debug_check_guards(self._h, C.byref(n)))
        return int(n.value), (lib().uwt_last_error(self._h).decode() if n.value else "")

    def debug_window_open(self):
        """Test instrumentation (uwt_debug_window_open): True while the early-preparation window of the last batch call is open."""
        out = C.c_int32(-1)
        self._chk(lib().uwt_debug_window_open(self._h, C.byref(out)))
        return bool(out.value)

    def update_params(self, **over):
        """Change solver constants of the live context (uwt_update_params)."""
        p = Params()
        self._chk(lib().uwt_get_params(self._h, C.byref(p)))
        _set_fields(p, over)
        self._chk(lib().uwt_update_params(self._h, C.byref(p)))
        self.params = p

    # -- frames
    def level_info(self, lvl):
        L = Level()
        self._chk(lib().uwt_level_info(self._h, lvl, C.byref(L)))
        return L

    def set_frame(self, slot, gray, depth=None):
        gray = np.asarray(gray)
        assert gray.dtype == np.uint8 and gray.shape == (self.h, self.w) and gray.strides[1] == 1
        dp, ds = None, 0
        if depth is not None:
            depth = np.asarray(depth)
            assert depth.dtype == np.uint16 and depth.shape == (self.h, self.w) and depth.strides[1] == 2
            dp, ds = _p(depth, C.c_uint16), depth.strides[0]
        self._chk(lib().uwt_set_frame(self._h, slot, _p(gray, C.c_uint8), gray.strides[0], dp, ds))

    def upload_frames(self, first_slot, gray, depth=None):
        gray = np.ascontiguousarray(gray, np.uint8)
        n = gray.shape[0]
        assert gray.shape[1:] == (self.h, self.w)
        dp = None
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            assert depth.shape == gray.shape
            dp = _p(depth, C.c_uint16)
        self._chk(lib().uwt_upload_frames(self._h, first_slot, n, _p(gray, C.c_uint8), dp))

    def upload_frames_async(self, first_slot, gray, depth=None):
        """gray / depth: page-locked arrays (pinned_empty) that stay untouched until the next sync()."""
        assert gray.flags["C_CONTIGUOUS"] and gray.dtype == np.uint8
        if depth is not None:
            assert depth.flags["C_CONTIGUOUS"] and depth.dtype == np.uint16
        self._chk(lib().uwt_upload_frames_async(self._h, first_slot, gray.shape[0], _p(gray, C.c_uint8),
                                                _p(depth, C.c_uint16) if depth is not None else None))

    def plane_device_ptr(self, slot, lvl, plane):
        out = C.c_void_p()
        self._chk(lib().uwt_plane_device_ptr(self._h, slot, lvl, plane, C.byref(out)))
        return out.value

    def get_plane(self, slot, lvl, plane):
        L = self.level_info(lvl)
        dt = {PLANE_IMAGE: np.uint8, PLANE_DEPTH: np.uint16, PLANE_GRADX: np.int16, PLANE_GRADY: np.int16}[plane]
        out = np.empty((L.img_h, L.img_w), dt)   # the level's image (larger than its point grid at odd sizes)
        self._chk(lib().uwt_get_plane(self._h, slot, lvl, plane, out.ctypes.data_as(C.c_void_p)))
        return out

    def build_pyramids(self, first_slot, n):
        self._chk(lib().uwt_build_pyramids(self._h, first_slot, n))

    def apply_gradient(self, first_slot, n):
        self._chk(lib().uwt_apply_gradient(self._h, first_slot, n))

    # -- tracking
    def estimate_pose_batch(self, ref_slots, tgt_slots, raise_on_pair_failure=False):
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        n = ref.size
        poses, stats = _result_buffers(n)
        st = lib().uwt_estimate_pose_batch(self._h, n, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(poses, C.c_float), stats)
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:n], _stats_list(stats, n)

    def track_batch_async(self, first_slot, n_frames, ref_slots, tgt_slots, d_poses_ptr, d_stats_ptr=None, grad_refs_only=True):
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        self._chk(lib().uwt_track_batch_async(self._h, first_slot, n_frames, int(grad_refs_only), ref.size, _p(ref, C.c_int32),
                                              _p(tgt, C.c_int32), d_poses_ptr, d_stats_ptr))

    def estimate_pose_batch_seeded(self, ref_slots, tgt_slots, seeds=None, handoff=None, raise_on_pair_failure=False):
        """estimate_pose_batch from start poses (uwt_estimate_pose_batch_seeded): seeds None (the identity) or [P, 7] float32 host
        poses; handoff: None / 0 / "reference", 1 / "keep", or a SeedOptions."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        n = ref.size
        poses, stats = _result_buffers(n)
        keep, sp = _host_seeds(seeds, n)
        st = lib().uwt_estimate_pose_batch_seeded(self._h, n, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(poses, C.c_float), stats, sp, _sopt(handoff))
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:n], _stats_list(stats, n)

    def track_batch_seeded_async(self, first_slot, n_frames, ref_slots, tgt_slots, d_poses_ptr, d_stats_ptr=None, grad_refs_only=True,
                                 d_seeds_ptr=None, handoff=None):
        """track_batch_async from seeds in device memory (uwt_track_batch_seeded_async): d_seeds_ptr None or P x 7 float32, e.g. the
        pose buffer of a call enqueued before, no wait between; it may overlap no output of this call."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        self._chk(lib().uwt_track_batch_seeded_async(self._h, first_slot, n_frames, int(grad_refs_only), ref.size, _p(ref, C.c_int32),
                                                     _p(tgt, C.c_int32), d_poses_ptr, d_stats_ptr, d_seeds_ptr, _sopt(handoff)))

    def predict_seeds_device_async(self, n, d_prev_ptr, d_cur_ptr, d_seed_ptr):
        """uwt_predict_seeds_device_async: seed = (cur * prev^-1) * cur per row, n x 7 float32 each in device memory, no wait."""
        self._chk(lib().uwt_predict_seeds_device_async(self._h, int(n), d_prev_ptr, d_cur_ptr, d_seed_ptr))

    def predict_seeds(self, prev, cur):
        """uwt_predict_seeds: the constant-velocity seeds (cur * prev^-1) * cur of host poses [n, 7], computed on the device"""
        a = np.ascontiguousarray(prev, np.float32).reshape(-1, 7)
        b = np.ascontiguousarray(cur, np.float32).reshape(-1, 7)
        if a.shape != b.shape:
            raise ValueError("predict_seeds: prev and cur differ in shape")
        out = np.empty_like(a)
        self._chk(lib().uwt_predict_seeds(self._h, a.shape[0], _p(a, C.c_float), _p(b, C.c_float), _p(out, C.c_float)))
        return out

    def track_batch_host_async(self, first_slot, n_frames, ref_slots, tgt_slots, h_poses, h_stats=None, grad_refs_only=True):
        """h_poses: pinned float32 [n, 7]; h_stats: pinned int32 [n, 4] or None.  Returns the ticket for wait_ticket()."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        t = C.c_int64()
        self._chk(lib().uwt_track_batch_host_async(self._h, first_slot, n_frames, int(grad_refs_only), ref.size, _p(ref, C.c_int32),
                                                   _p(tgt, C.c_int32), _p(h_poses, C.c_float),
                                                   h_stats.ctypes.data if h_stats is not None else None, C.byref(t)))
        return t.value

    def wait_ticket(self, ticket):
        self._chk(lib().uwt_wait_ticket(self._h, ticket))

    def sync(self):
        self._chk(lib().uwt_sync(self._h))

    def set_deferred(self, on=True):
        """build_pyramids / apply_gradient return once enqueued; the calls that deliver results wait as before."""
        self._chk(lib().uwt_set_deferred(self._h, int(on)))

    def stream(self):
        out = C.c_void_p()
        self._chk(lib().uwt_stream(self._h, C.byref(out)))
        return out.value

    def profile_enable(self, on=True):
        self._chk(lib().uwt_profile_enable(self._h, int(on)))

    def profile_read(self):
        ms, n, px = C.c_double(), C.c_int64(), C.c_int64()
        self._chk(lib().uwt_profile_read(self._h, C.byref(ms), C.byref(n), C.byref(px)))
        return ms.value, n.value, px.value

    def profile_read_levels(self):
        """[(ms, launches)] by pyramid level for the residual launches since profiling was enabled."""
        n = self.params.n_levels
        ms = (C.c_double * n)()
        cnt = (C.c_int64 * n)()
        self._chk(lib().uwt_profile_read_levels(self._h, ms, cnt, n))
        return [(ms[l], cnt[l]) for l in range(n)]

    def profile_clock(self):
        """Shader clock (GHz) inside the last profiled residual launch."""
        ghz = C.c_double()
        self._chk(lib().uwt_profile_clock(self._h, C.byref(ghz)))
        return ghz.value

    # -- per-stage entry points
    def _half(self, fn, img, dtype, size):
        """One of the four halving entries: img as dtype, out of size(h) x size(w)"""
        img = np.ascontiguousarray(img, dtype)
        h, w = img.shape
        out = np.empty((size(h), size(w)), dtype)
        self._chk(fn(self._h, img.ctypes.data, w, h, out.ctypes.data))
        return out

    def halve_u8(self, img):
        return self._half(lib().uwt_halve_u8, img, np.uint8, lambda n: n // 2)

    def halve_u16(self, img):
        return self._half(lib().uwt_halve_u16, img, np.uint16, lambda n: n // 2)

    def resize_half_u8(self, img):
        """cv::resize(img, Size(), 0.5, 0.5) on any size."""
        return self._half(lib().uwt_resize_half_u8, img, np.uint8, lib().uwt_half_size)

    def resize_half_u16(self, img):
        return self._half(lib().uwt_resize_half_u16, img, np.uint16, lib().uwt_half_size)

    def scharr3(self, img):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        gx = np.empty((h, w), np.int16)
        gy = np.empty((h, w), np.int16)
        self._chk(lib().uwt_scharr3(self._h, _p(img, C.c_uint8), w, h, _p(gx, C.c_int16), _p(gy, C.c_int16)))
        return gx, gy

    def warp(self, lvl, pts, pose):
        pts = np.ascontiguousarray(pts, np.float32)
        pose = np.ascontiguousarray(pose, np.float32)
        out = np.empty_like(pts)
        self._chk(lib().uwt_warp(self._h, lvl, _p(pts, C.c_float), pts.shape[0], _p(pose, C.c_float), _p(out, C.c_float)))
        return out

    def residual_jacobian(self, ref_slot, tgt_slot, lvl, pose, dump=True):
        pose = np.ascontiguousarray(pose, np.float32)
        L = self.level_info(lvl)
        n = L.w * L.h
        acc = Accum()
        J = np.empty((n, 6), np.float32) if dump else None
        r = np.empty(n, np.float32) if dump else None
        v = np.empty(n, np.uint8) if dump else None
        self._chk(lib().uwt_residual_jacobian(self._h, ref_slot, tgt_slot, lvl, _p(pose, C.c_float), C.byref(acc),
                                              _p(J, C.c_float) if dump else None, _p(r, C.c_float) if dump else None,
                                              _p(v, C.c_uint8) if dump else None))
        return dict(_accum_fields(acc), J=J, r=r, valid=v)

    def ls_accumulate(self, J, r, w=None, divide=False):
        return self._ls_accumulate(lib().uwt_ls_accumulate, J, r, w, divide)

    def ls_accumulate_sse(self, J, r, w=None, divide=False, count_quirk=True):
        return self._ls_accumulate(lib().uwt_ls_accumulate_sse, J, r, w, divide, int(count_quirk))

    def _ls_accumulate(self, fn, J, r, w, divide, *quirk):
        J = np.ascontiguousarray(J, np.float32)
        r = np.ascontiguousarray(r, np.float32)
        A = np.empty(36, np.float32)
        b = np.empty(6, np.float32)
        err, cnt = C.c_float(), C.c_int32()
        wp = None
        if w is not None:
            w = np.ascontiguousarray(w, np.float32)
            wp = _p(w, C.c_float)
        self._chk(fn(self._h, _p(J, C.c_float), _p(r, C.c_float), wp, r.size, int(divide), *quirk, _p(A, C.c_float), _p(b, C.c_float),
                     C.byref(err), C.byref(cnt)))
        return A.reshape(6, 6), b, err.value, cnt.value

    def se3_exp(self, xi):
        xi = np.ascontiguousarray(xi, np.float32)
        out = np.empty(7, np.float32)
        self._chk(lib().uwt_se3_exp(self._h, _p(xi, C.c_float), _p(out, C.c_float)))
        return out

    def se3_mul(self, a, b):
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        out = np.empty(7, np.float32)
        self._chk(lib().uwt_se3_mul(self._h, _p(a, C.c_float), _p(b, C.c_float), _p(out, C.c_float)))
        return out

    def se3_matrix(self, pose):
        pose = np.ascontiguousarray(pose, np.float32)
        out = np.empty(16, np.float32)
        self._chk(lib().uwt_se3_matrix(self._h, _p(pose, C.c_float), _p(out, C.c_float)))
        return out.reshape(4, 4)

    def se3_handoff(self, pose, scale_t=0):
        pose = np.array(pose, np.float32)
        self._chk(lib().uwt_se3_handoff(self._h, _p(pose, C.c_float), int(scale_t)))
        return pose

    def solve_delta(self, A, b):
        A = np.ascontiguousarray(A, np.float32).reshape(36)
        b = np.ascontiguousarray(b, np.float32)
        d = np.empty(6, np.float32)
        Ai = np.empty(36, np.float32)
        ok = C.c_int32()
        self._chk(lib().uwt_solve_delta(self._h, _p(A, C.c_float), _p(b, C.c_float), _p(d, C.c_float), _p(Ai, C.c_float),
                                        C.byref(ok)))
        return d, Ai.reshape(6, 6), bool(ok.value)

    def gn_update_records(self, form, records, states, count, pair_base=0, k=0, max_iters=50, early_exit=1, epsilon=1e-3, gain=50.0,
                          general=0):
        """uwt_gn_update_records (test surface): one update of pairs pair_base.. from explicit records.  records: rows x stride x 64
        uint32 words, states: rows records of PAIR_STATE_DTYPE (rows = pair_base + the pairs to update); form 0 the block form, 1 the
        tail form.  Returns (states_out, active, tickets)."""
        records = np.ascontiguousarray(records, np.uint32)
        states = np.ascontiguousarray(states, PAIR_STATE_DTYPE).reshape(-1)
        if records.ndim != 3 or records.shape[2] != 64 or records.shape[0] != states.size:
            raise ValueError("records: rows x stride x 64 words, one row per state")
        rows, stride = records.shape[0], records.shape[1]
        out = np.full(rows, 0, PAIR_STATE_DTYPE)
        tickets = np.full(rows, 0xffffffff, np.uint32)
        active = C.c_int32(-1)
        self._chk(lib().uwt_gn_update_records(self._h, int(form), rows - int(pair_base), int(pair_base), stride, int(count),
                                              _p(records, C.c_uint32), states.ctypes.data_as(C.POINTER(PairState)), int(k), int(max_iters),
                                              int(early_exit), epsilon, gain, int(general),
                                              out.ctypes.data_as(C.POINTER(PairState)), C.byref(active), _p(tickets, C.c_uint32)))
        return out, active.value, tickets

    def accumulate_trajectory(self, poses, start=None, t_scale=1.0, reference_axes=False, scan=False):
        """scan=True: the parallel prefix product (equal to the sequential form to float rounding, not bit for bit)."""
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        start = np.array([0, 0, 0, 1, 0, 0, 0], np.float32) if start is None else np.ascontiguousarray(start, np.float32)
        out = np.empty_like(poses)
        fn = lib().uwt_accumulate_trajectory_scan if scan else lib().uwt_accumulate_trajectory
        self._chk(fn(self._h, _p(poses, C.c_float), poses.shape[0], _p(start, C.c_float), t_scale, int(bool(reference_axes)),
                     _p(out, C.c_float)))
        return out

    def estimate_pose_points(self, ref_slot, tgt_slot, tables):
        """tables: {level: n x 4 float32 array}"""
        nl = self.params.n_levels
        arrs = [None] * nl
        ptrs = (C.POINTER(C.c_float) * MAX_LEVELS)()
        counts = (C.c_int32 * MAX_LEVELS)()
        for l, t in tables.items():
            arrs[l] = np.ascontiguousarray(t, np.float32).reshape(-1, 4)
            counts[l] = arrs[l].shape[0]
            if arrs[l].shape[0]:
                ptrs[l] = _p(arrs[l], C.c_float)
        pose = np.empty(7, np.float32)
        st = Stats()
        rc = lib().uwt_estimate_pose_points(self._h, ref_slot, tgt_slot, ptrs, counts, _p(pose, C.c_float), C.byref(st))
        self._chk(rc, allow=(ERR_PAIR_FAILED,))
        return pose, _stats_list([st], 1)[0]

    def robust_weights(self, residuals, kind=1, want_weights=True):
        """MedianMat / MedianAbsoluteDeviation / IdentityWeights (kind 0) / TukeyFunctionWeights (kind 1) of an N x 1 vector.
        Returns (weights or None, median, MAD)."""
        r = np.ascontiguousarray(residuals, np.float32).reshape(-1)
        w = np.empty(r.size, np.float32) if want_weights else None
        med, mad = C.c_float(), C.c_float()
        self._chk(lib().uwt_robust_weights(self._h, _p(r, C.c_float), r.size, int(kind), _p(w, C.c_float) if want_weights else None,
                                           C.byref(med), C.byref(mad)))
        return w, med.value, mad.value

    def gradient_magnitude(self, slot, lvl):
        L = self.level_info(lvl)
        out = np.empty((L.img_h, L.img_w), np.uint8)   # gradient_[lvl]: the level's image
        self._chk(lib().uwt_gradient_magnitude(self._h, slot, lvl, _p(out, C.c_uint8)))
        return out

    def obtain_candidate_points(self, slot, lvl, threshold=20.0, cap=None):
        L = self.level_info(lvl)
        cap = L.w * L.h if cap is None else cap
        pts = np.empty((max(cap, 1), 4), np.float32)
        cnt = C.c_int32()
        self._chk(lib().uwt_obtain_candidate_points(self._h, slot, lvl, threshold, _p(pts, C.c_float), cap, C.byref(cnt)))
        return pts[:min(cnt.value, cap)].copy(), cnt.value

    def obtain_candidate_points_batch(self, first_slot, n_frames, lvl, threshold=20.0, cap=None):
        """Returns (list of [count_f, 4] arrays, counts)."""
        L = self.level_info(lvl)
        cap = L.w * L.h if cap is None else cap
        pts = np.empty((n_frames, max(cap, 1), 4), np.float32)
        cnt = np.zeros(n_frames, np.int32)
        self._chk(lib().uwt_obtain_candidate_points_batch(self._h, first_slot, n_frames, lvl, threshold, _p(pts, C.c_float), cap,
                                                          _p(cnt, C.c_int32)))
        return [pts[f, :min(int(cnt[f]), cap)].copy() for f in range(n_frames)], cnt

    def obtain_patch_points(self, slot, keypoints, cap=200 * 144):
        kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
        pts = np.empty((max(cap, 1), 4), np.float32)
        cnt = C.c_int32()
        self._chk(lib().uwt_obtain_patch_points(self._h, slot, _p(kp, C.c_float), kp.shape[0], _p(pts, C.c_float), cap,
                                                C.byref(cnt)))
        return pts[:min(cnt.value, cap)].copy(), cnt.value

    @staticmethod
    def _keypoint_block(keypoints_list):
        """A list of (n_i, 2) key point arrays as the batch calls take them: [P, 200, 2] float32 (the first 200 of each, zero
        padded) and the counts n_i."""
        kps = [np.ascontiguousarray(k, np.float32).reshape(-1, 2) for k in keypoints_list]
        block = np.zeros((len(kps), 200, 2), np.float32)
        n = np.zeros(len(kps), np.int32)
        for i, k in enumerate(kps):
            m = min(k.shape[0], 200)
            block[i, :m] = k[:m]
            n[i] = k.shape[0]
        return block, n

    def obtain_patch_points_batch(self, slots, keypoints_list, cap=200 * 144):
        """Tracker::ObtainPatchesPoints for many frames at once.  Returns (list of [min(count_f, cap), 4] arrays, counts)."""
        sl = np.ascontiguousarray(slots, np.int32)
        kp, n = self._keypoint_block(keypoints_list)
        pts = np.empty((max(sl.size, 1), max(cap, 1), 4), np.float32)
        cnt = np.zeros(max(sl.size, 1), np.int32)
        self._chk(lib().uwt_obtain_patch_points_batch(self._h, sl.size, _p(sl, C.c_int32), _p(kp, C.c_float), _p(n, C.c_int32),
                                                      _p(pts, C.c_float), cap, _p(cnt, C.c_int32)))
        return [pts[f, :min(int(cnt[f]), cap)].copy() for f in range(sl.size)], cnt[:sl.size]

    @staticmethod
    def _table_entry(plain, opt, weights, sampler):
        """(entry, its options argument) of a table tracker: the plain entry and no argument when neither weights nor sampler is
        given, else the _opt entry and the uwt_table_options of the two"""
        if weights is None and sampler is None:
            return plain, ()
        return opt, (C.byref(table_options(weights, sampler)),)

    def estimate_pose_features_batch(self, ref_slots, tgt_slots, keypoints_list, raise_on_pair_failure=False, weights=None,
                                     sampler=None):
        """System::Tracking's live call for many pairs: keypoints_list[i] are the key points of the frame in ref_slots[i].
        weights / sampler (either given): the call's own robust weights and sampler, uwt_estimate_pose_features_batch_opt.
        Returns (poses [P, 7], per-pair stats)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        kp, n = self._keypoint_block(keypoints_list)
        poses, stats = _result_buffers(ref.size)
        fn, opt = self._table_entry(lib().uwt_estimate_pose_features_batch, lib().uwt_estimate_pose_features_batch_opt, weights, sampler)
        st = fn(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(kp, C.c_float), _p(n, C.c_int32), *opt, _p(poses, C.c_float), stats)
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:ref.size], _stats_list(stats, ref.size)

    def track_features_batch_async(self, ref_slots, tgt_slots, keypoints_list, d_poses_ptr, d_stats_ptr=None, weights=None,
                                   sampler=None):
        """The same enqueued on the context stream, results in device memory (d_poses_ptr: P x 7 float32, d_stats_ptr: P x 4
        int32-sized uwt_stats or None); sync() to wait."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        kp, n = self._keypoint_block(keypoints_list)
        fn, opt = self._table_entry(lib().uwt_track_features_batch_async, lib().uwt_track_features_batch_opt_async, weights, sampler)
        self._chk(fn(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(kp, C.c_float), _p(n, C.c_int32), *opt, d_poses_ptr, d_stats_ptr))

    def estimate_pose_features_batch_seeded(self, ref_slots, tgt_slots, keypoints_list, seeds=None, handoff=None, weights=None,
                                            sampler=None, raise_on_pair_failure=False):
        """estimate_pose_features_batch from start poses (uwt_estimate_pose_features_batch_seeded; seeds, handoff: as
        estimate_pose_batch_seeded)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        kp, n = self._keypoint_block(keypoints_list)
        poses, stats = _result_buffers(ref.size)
        keep, sp = _host_seeds(seeds, ref.size)
        st = lib().uwt_estimate_pose_features_batch_seeded(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(kp, C.c_float),
                                                           _p(n, C.c_int32), C.byref(table_options(weights, sampler)),
                                                           _p(poses, C.c_float), stats, sp, _sopt(handoff))
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:ref.size], _stats_list(stats, ref.size)

    def track_features_batch_seeded_async(self, ref_slots, tgt_slots, keypoints_list, d_poses_ptr, d_stats_ptr=None, d_seeds_ptr=None,
                                          handoff=None, weights=None, sampler=None):
        """track_features_batch_async from seeds in device memory (uwt_track_features_batch_seeded_async)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        kp, n = self._keypoint_block(keypoints_list)
        self._chk(lib().uwt_track_features_batch_seeded_async(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), _p(kp, C.c_float),
                                                              _p(n, C.c_int32), C.byref(table_options(weights, sampler)), d_poses_ptr,
                                                              d_stats_ptr, d_seeds_ptr, _sopt(handoff)))

    def estimate_pose_candidates_batch_seeded(self, ref_slots, tgt_slots, seeds=None, handoff=None, threshold=20.0, weights=None,
                                              sampler=None, raise_on_pair_failure=False):
        """estimate_pose_candidates_batch from start poses (uwt_estimate_pose_candidates_batch_seeded); the weights and the sampler
        are the call's, as in the _opt entry."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        poses, stats = _result_buffers(ref.size)
        keep, sp = _host_seeds(seeds, ref.size)
        st = lib().uwt_estimate_pose_candidates_batch_seeded(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), threshold,
                                                             C.byref(table_options(weights, sampler)), _p(poses, C.c_float), stats, sp,
                                                             _sopt(handoff))
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:ref.size], _stats_list(stats, ref.size)

    def track_candidates_batch_seeded_async(self, ref_slots, tgt_slots, d_poses_ptr, d_stats_ptr=None, d_seeds_ptr=None, handoff=None,
                                            threshold=20.0, weights=None, sampler=None):
        """track_candidates_batch_async from seeds in device memory (uwt_track_candidates_batch_seeded_async)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        self._chk(lib().uwt_track_candidates_batch_seeded_async(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), threshold,
                                                                C.byref(table_options(weights, sampler)), d_poses_ptr, d_stats_ptr,
                                                                d_seeds_ptr, _sopt(handoff)))

    def estimate_pose_candidates_batch(self, ref_slots, tgt_slots, threshold=20.0, raise_on_pair_failure=False, weights=None,
                                       sampler=None):
        """Semi-dense tracking for many pairs: Tracker::ObtainCandidatePoints(previous) on every iterated level, then EstimatePose
        (previous, current) over those tables, under the context's params.  weights / sampler (either given): the call's own robust
        weights and sampler, uwt_estimate_pose_candidates_batch_opt (the context's are then not looked at).
        Returns (poses [P, 7], per-pair stats)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        poses, stats = _result_buffers(ref.size)
        fn, opt = self._table_entry(lib().uwt_estimate_pose_candidates_batch, lib().uwt_estimate_pose_candidates_batch_opt, weights, sampler)
        st = fn(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), threshold, *opt, _p(poses, C.c_float), stats)
        self._chk_pairs(st, raise_on_pair_failure)
        return poses[:ref.size], _stats_list(stats, ref.size)

    def track_candidates_batch_async(self, ref_slots, tgt_slots, d_poses_ptr, d_stats_ptr=None, threshold=20.0, weights=None,
                                     sampler=None):
        """The same enqueued on the context stream, results in device memory (d_poses_ptr: P x 7 float32, d_stats_ptr: P x 4
        int32-sized uwt_stats or None); sync() to wait."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        fn, opt = self._table_entry(lib().uwt_track_candidates_batch_async, lib().uwt_track_candidates_batch_opt_async, weights, sampler)
        self._chk(fn(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), threshold, *opt, d_poses_ptr, d_stats_ptr))

    @staticmethod
    def _descriptor_block(pairs, packed, cap):
        """The matching calls' inputs: either `pairs`, a list of per-pair (A [n, dim], B [m, dim]) arrays, packed here into the
        fixed-stride form, or `packed` = (query [P, cap, dim], n_query [P], train [P, cap, dim], n_train [P]) as it is.  dtype
        decides the norm: float32 is L2, uint8 is Hamming.  Returns (norm, dim, cap, query, n_query, train, n_train)."""
        if packed is not None:
            q, nq, t, nt = packed
            if q.dtype not in (np.float32, np.uint8) or t.dtype != q.dtype or q.ndim != 3 or q.shape != t.shape:
                raise ValueError("packed descriptors: two [P, cap, dim] arrays of float32 (L2) or uint8 (Hamming)")
            q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
            nq, nt = np.ascontiguousarray(nq, np.int32), np.ascontiguousarray(nt, np.int32)
            return (NORM_L2 if q.dtype == np.float32 else NORM_HAMMING), q.shape[2], q.shape[1], q, nq, t, nt
        pairs = [(np.asarray(a), np.asarray(b)) for a, b in pairs]
        dtype = pairs[0][0].dtype
        if dtype not in (np.float32, np.uint8) or any(a.dtype != dtype or b.dtype != dtype or a.ndim != 2 or b.ndim != 2 or
                                                      a.shape[1] != pairs[0][0].shape[1] or b.shape[1] != a.shape[1] for a, b in pairs):
            raise ValueError("descriptor pairs: (A [n, dim], B [m, dim]) arrays of one dim, all float32 (L2) or all uint8 (Hamming)")
        dim = pairs[0][0].shape[1]
        cap = max([cap or 1] + [max(a.shape[0], b.shape[0]) for a, b in pairs])
        q, t = np.zeros((len(pairs), cap, dim), dtype), np.zeros((len(pairs), cap, dim), dtype)
        nq, nt = np.zeros(len(pairs), np.int32), np.zeros(len(pairs), np.int32)
        for i, (a, b) in enumerate(pairs):
            q[i, :a.shape[0]], t[i, :b.shape[0]] = a, b
            nq[i], nt[i] = a.shape[0], b.shape[0]
        return (NORM_L2 if dtype == np.float32 else NORM_HAMMING), dim, cap, q, nq, t, nt

    def knn_match_batch(self, pairs=None, cap=None, packed=None):
        """matcher->knnMatch(A, B, matches, 2) for many pairs (uwt_knn_match_batch).  Returns one KNN2 record array per pair, a row
        per query descriptor: idx0, idx1 (-1: no such neighbour), d0, d1."""
        norm, dim, cap, q, nq, t, nt = self._descriptor_block(pairs, packed, cap)
        out = np.zeros((nq.size, cap), KNN2)
        self._chk(lib().uwt_knn_match_batch(self._h, nq.size, norm, dim, q.ctypes.data, _p(nq, C.c_int32), t.ctypes.data,
                                            _p(nt, C.c_int32), cap, out.ctypes.data))
        return [out[i, :nq[i]].copy() for i in range(nq.size)]

    def match_descriptors_batch(self, pairs=None, ratio=0.65, cap=None, packed=None):
        """knnMatch both ways, ratioTest both ways and symmetryTest for many pairs (uwt_match_descriptors_batch).  Returns one MATCH
        record array per pair (query_idx, train_idx, distance), ascending query_idx."""
        norm, dim, cap, q, nq, t, nt = self._descriptor_block(pairs, packed, cap)
        out = np.zeros((nq.size, cap), MATCH)
        cnt = np.zeros(nq.size, np.int32)
        self._chk(lib().uwt_match_descriptors_batch(self._h, nq.size, norm, dim, q.ctypes.data, _p(nq, C.c_int32), t.ctypes.data,
                                                    _p(nt, C.c_int32), cap, ratio, out.ctypes.data, _p(cnt, C.c_int32)))
        return [out[i, :cnt[i]].copy() for i in range(nq.size)]

    def match_descriptors_batch_async(self, d_matches_ptr, d_counts_ptr, pairs=None, ratio=0.65, cap=None, packed=None):
        """The same enqueued on the context stream, results in device memory (d_matches_ptr: P x cap MATCH records, d_counts_ptr: P
        int32); sync() to wait.  Returns cap.  Packed arrays from pinned_empty must stay untouched until the copy has run."""
        norm, dim, cap, q, nq, t, nt = self._descriptor_block(pairs, packed, cap)
        self._chk(lib().uwt_match_descriptors_batch_async(self._h, nq.size, norm, dim, q.ctypes.data, _p(nq, C.c_int32), t.ctypes.data,
                                                          _p(nt, C.c_int32), cap, ratio, d_matches_ptr, d_counts_ptr))
        return cap

    @staticmethod
    def _ransac_block(pairs, cap, kp_cap):
        """A list of per-pair (matches, kp_prev [n, 2], kp_cur [m, 2]) in the fixed-stride form of the RANSAC calls: (cap, kp_cap,
        matches [P, cap] MATCH, n_matches [P], kp_prev [P, kp_cap, 2], n_kp_prev [P], kp_cur [P, kp_cap, 2], n_kp_cur [P])."""
        pairs = [(np.ascontiguousarray(m, MATCH).reshape(-1), np.ascontiguousarray(a, np.float32).reshape(-1, 2),
                  np.ascontiguousarray(b, np.float32).reshape(-1, 2)) for m, a, b in pairs]
        cap = max([cap or 1] + [len(m) for m, _, _ in pairs])
        kp_cap = max([kp_cap or 1] + [max(len(a), len(b)) for _, a, b in pairs])
        P = len(pairs)
        mt, nm = np.zeros((P, cap), MATCH), np.zeros(P, np.int32)
        k0, k1 = np.zeros((P, kp_cap, 2), np.float32), np.zeros((P, kp_cap, 2), np.float32)
        n0, n1 = np.zeros(P, np.int32), np.zeros(P, np.int32)
        for i, (m, a, b) in enumerate(pairs):
            mt[i, :len(m)], k0[i, :len(a)], k1[i, :len(b)] = m, a, b
            nm[i], n0[i], n1[i] = len(m), len(a), len(b)
        return cap, kp_cap, mt, nm, k0, n0, k1, n1

    def ransac_inliers_batch(self, pairs, params=None, cap=None, kp_cap=None):
        """RobustMatcher::ransacTest for many pairs (uwt_ransac_inliers_batch): pairs is a list of (matches, kp_prev, kp_cur).
        Returns one (mask uint8 [n], good matches MATCH [count], info RANSAC_INFO record) per pair."""
        cap, kp_cap, mt, nm, k0, n0, k1, n1 = self._ransac_block(pairs, cap, kp_cap)
        P = nm.size
        mask, good = np.zeros((P, cap), np.uint8), np.zeros((P, cap), MATCH)
        cnt, info = np.zeros(P, np.int32), np.zeros(P, RANSAC_INFO)
        self._chk(lib().uwt_ransac_inliers_batch(self._h, P, mt.ctypes.data, _p(nm, C.c_int32), cap, _p(k0, C.c_float), _p(n0, C.c_int32),
                                                 _p(k1, C.c_float), _p(n1, C.c_int32), kp_cap, _ref(params), mask.ctypes.data,
                                                 good.ctypes.data, _p(cnt, C.c_int32), info.ctypes.data))
        return [(mask[i, :nm[i]].copy(), good[i, :cnt[i]].copy(), info[i].copy()) for i in range(P)]

    def ransac_inliers_batch_async(self, d_matches_ptr, d_n_matches_ptr, cap, keypoints, d_mask_ptr, d_good_ptr, d_counts_ptr,
                                   d_info_ptr, params=None, kp_cap=None):
        """The same with the matches and their counts in device memory (d_matches_ptr: P x cap MATCH, d_n_matches_ptr: P int32, as
        match_descriptors_batch_async left them) and the results left there (d_mask_ptr: P x cap bytes, d_good_ptr: P x cap MATCH,
        d_counts_ptr: P int32, d_info_ptr: P RANSAC_INFO); keypoints: a list of per-pair (kp_prev, kp_cur).  sync() to wait.
        Returns kp_cap."""
        _, kp_cap, _, _, k0, n0, k1, n1 = self._ransac_block([(np.zeros(0, MATCH), a, b) for a, b in keypoints], None, kp_cap)
        self._chk(lib().uwt_ransac_inliers_batch_async(self._h, n0.size, d_matches_ptr, d_n_matches_ptr, cap, _p(k0, C.c_float),
                                                       _p(n0, C.c_int32), _p(k1, C.c_float), _p(n1, C.c_int32), kp_cap, _ref(params),
                                                       d_mask_ptr, d_good_ptr, d_counts_ptr, d_info_ptr))
        return kp_cap

    # ---- SURF and ORB detection and description: one helper per form; fn: the library's entry, dtype / row: a descriptor row
    def _detect_describe(self, fn, dtype, row, slots, params, cap, describe, out):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        F = slots.size
        if out is None:
            out = (np.zeros((F, cap), KEYPOINT), np.zeros((F, cap, row), dtype) if describe else None, np.zeros(F, np.int32))
        kp, desc, cnt = out
        self._chk(fn(self._h, F, _p(slots, C.c_int32), _ref(params), cap, kp.ctypes.data, desc.ctypes.data if desc is not None else None,
                     _p(cnt, C.c_int32)))
        return [(kp[i, :cnt[i]].copy(), desc[i, :cnt[i]].copy() if desc is not None else None) for i in range(F)]

    def _detect_describe_async(self, fn, slots, d_kp_ptr, d_desc_ptr, d_counts_ptr, params, cap):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        self._chk(fn(self._h, slots.size, _p(slots, C.c_int32), _ref(params), cap, d_kp_ptr, d_desc_ptr, d_counts_ptr))

    def _describe(self, fn, dtype, row, slots, keypoints_list, params, cap, out):
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        kin = [np.ascontiguousarray(k, KEYPOINT).reshape(-1) for k in keypoints_list]
        cap = max([cap or 1] + [len(k) for k in kin])
        F = slots.size
        kp, n = np.zeros((F, cap), KEYPOINT), np.zeros(F, np.int32)
        for i, k in enumerate(kin):
            kp[i, :len(k)], n[i] = k, len(k)
        res, desc = out if out is not None else (np.zeros((F, cap), KEYPOINT), np.zeros((F, cap, row), dtype))
        self._chk(fn(self._h, F, _p(slots, C.c_int32), _ref(params), kp.ctypes.data, _p(n, C.c_int32), cap, res.ctypes.data,
                     desc.ctypes.data))
        return [(res[i, :n[i]].copy(), desc[i, :n[i]].copy()) for i in range(F)]

    def surf_detect_describe_batch(self, slots, params=None, cap=UWT_MATCH_MAX_ROWS, describe=True, out=None):
        """SURF key points and descriptors of the frames resident in `slots` (uwt_surf_detect_describe_batch).  Returns one
        (key points KEYPOINT [n], descriptors float32 [n, 64] or None) per frame.  out: (kp [F, cap] KEYPOINT, desc [F, cap, 64]
        float32 or None, counts [F] int32) to be written in place — the rows past a frame's count stay as they are."""
        return self._detect_describe(lib().uwt_surf_detect_describe_batch, np.float32, 64, slots, params, cap, describe, out)

    def surf_detect_describe_batch_async(self, slots, d_kp_ptr, d_desc_ptr, d_counts_ptr, params=None, cap=UWT_MATCH_MAX_ROWS):
        """The same enqueued on the context stream, results in device memory (d_kp_ptr: F x cap KEYPOINT, d_desc_ptr: F x cap x 64
        float32 or None, d_counts_ptr: F int32); sync() to wait."""
        self._detect_describe_async(lib().uwt_surf_detect_describe_batch_async, slots, d_kp_ptr, d_desc_ptr, d_counts_ptr, params, cap)

    def surf_describe_batch(self, slots, keypoints_list, params=None, cap=None):
        """Orientation and descriptors at the caller's key points (uwt_surf_describe_batch: useProvidedKeypoints): keypoints_list
        holds one KEYPOINT array per frame (x, y, size are read).  Returns one (key points with directions, descriptors) per frame."""
        return self._describe(lib().uwt_surf_describe_batch, np.float32, 64, slots, keypoints_list, params, cap, None)

    def orb_set_pattern(self, pattern=None):
        """Loads a sampling pattern (int8 [256, 4]; uwt_orb_set_pattern) for the ORB calls that follow; None restores the default."""
        if pattern is not None:
            pattern = np.ascontiguousarray(pattern, np.int8).reshape(1024)
        self._chk(lib().uwt_orb_set_pattern(self._h, _p(pattern, C.c_int8) if pattern is not None else None))

    def orb_detect_describe_batch(self, slots, params=None, cap=UWT_MATCH_MAX_ROWS, describe=True, out=None):
        """ORB key points and descriptors of the frames resident in `slots` (uwt_orb_detect_describe_batch).  Returns one
        (key points KEYPOINT [n], descriptors uint8 [n, 32] or None) per frame.  out: (kp [F, cap] KEYPOINT, desc [F, cap, 32]
        uint8 or None, counts [F] int32) to be written in place — the rows past a frame's count stay as they are."""
        return self._detect_describe(lib().uwt_orb_detect_describe_batch, np.uint8, 32, slots, params, cap, describe, out)

    def orb_detect_describe_batch_async(self, slots, d_kp_ptr, d_desc_ptr, d_counts_ptr, params=None, cap=UWT_MATCH_MAX_ROWS):
        """The same enqueued on the context stream, results in device memory (d_kp_ptr: F x cap KEYPOINT, d_desc_ptr: F x cap x 32
        bytes or None, d_counts_ptr: F int32); sync() to wait."""
        self._detect_describe_async(lib().uwt_orb_detect_describe_batch_async, slots, d_kp_ptr, d_desc_ptr, d_counts_ptr, params, cap)

    def orb_describe_batch(self, slots, keypoints_list, params=None, cap=None, out=None):
        """Direction and descriptors at the caller's key points (uwt_orb_describe_batch: useProvidedKeypoints): keypoints_list
        holds one KEYPOINT array per frame (x, y, octave are read).  Returns one (key points with directions, descriptors) per
        frame.  out: (kp [F, cap] KEYPOINT, desc [F, cap, 32] uint8) to be written in place."""
        return self._describe(lib().uwt_orb_describe_batch, np.uint8, 32, slots, keypoints_list, params, cap, out)

    def orb_layer(self, slot, level):
        """One layer of the ORB scale pyramid of a slot (uwt_orb_layer): uint8 [h_l, w_l]"""
        out = np.zeros(max(1, self.params.height * self.params.width), np.uint8)
        lw, lh = C.c_int32(0), C.c_int32(0)
        self._chk(lib().uwt_orb_layer(self._h, slot, level, _p(out, C.c_uint8), C.byref(lw), C.byref(lh)))
        return out[:lw.value * lh.value].reshape(lh.value, lw.value)

    def orb_fast_scores(self, slot, level):
        """The dense FAST score map of a layer, after the border rule and before suppression (uwt_orb_fast_scores): int32 [h_l, w_l]"""
        lw, lh = orb_layer_size(self.params.width, self.params.height, level)
        out = np.zeros(max(1, lw * lh), np.int32)
        self._chk(lib().uwt_orb_fast_scores(self._h, slot, level, _p(out, C.c_int32)))
        return out[:lw * lh].reshape(lh, lw)

    def orb_harris(self, slot, level, xy):
        """The integer Harris measure at pixels (x, y) of a layer (uwt_orb_harris): int64 [n]"""
        xy = np.ascontiguousarray(xy, np.int32).reshape(-1, 2)
        out = np.zeros(len(xy), np.int64)
        self._chk(lib().uwt_orb_harris(self._h, slot, level, _p(xy, C.c_int32), len(xy), _p(out, C.c_int64)))
        return out

    def tracking_batch(self, ref_slots, tgt_slots, prev=None, params=None, cap=2048, out=None, raise_on_pair_failure=False):
        """System::Tracking for many pairs in one device-resident call with SURF and the L2 matcher (uwt_tracking_batch; params:
        TrackingParams); arguments and result: _tracking_batch."""
        return self._tracking_batch(lib().uwt_tracking_batch, ref_slots, tgt_slots, prev, params, cap, out, raise_on_pair_failure)

    def tracking_orb_batch(self, ref_slots, tgt_slots, prev=None, params=None, cap=2048, out=None, raise_on_pair_failure=False):
        """tracking_batch for RobustMatcher(1): ORB and the Hamming matcher (uwt_tracking_orb_batch; params: TrackingOrbParams), under
        the context's pattern in force.  Arguments and result as there."""
        return self._tracking_batch(lib().uwt_tracking_orb_batch, ref_slots, tgt_slots, prev, params, cap, out, raise_on_pair_failure)

    def tracking_orb_batch_async(self, ref_slots, tgt_slots, io, params=None, cap=2048):
        """tracking_batch_async for RobustMatcher(1) (uwt_tracking_orb_batch_async)."""
        self._tracking_batch_async(lib().uwt_tracking_orb_batch_async, ref_slots, tgt_slots, io, params, cap)

    def tracking_batch_seeded(self, ref_slots, tgt_slots, prev=None, params=None, cap=2048, out=None, raise_on_pair_failure=False,
                              seeds=None, handoff=None):
        """tracking_batch from host seeds [P, 7] (uwt_tracking_batch_seeded)."""
        return self._tracking_batch(lib().uwt_tracking_batch_seeded, ref_slots, tgt_slots, prev, params, cap, out, raise_on_pair_failure,
                                    (seeds, handoff))

    def tracking_orb_batch_seeded(self, ref_slots, tgt_slots, prev=None, params=None, cap=2048, out=None, raise_on_pair_failure=False,
                                  seeds=None, handoff=None):
        """tracking_orb_batch from host seeds [P, 7] (uwt_tracking_orb_batch_seeded)."""
        return self._tracking_batch(lib().uwt_tracking_orb_batch_seeded, ref_slots, tgt_slots, prev, params, cap, out,
                                    raise_on_pair_failure, (seeds, handoff))

    def _tracking_batch(self, fn, ref_slots, tgt_slots, prev, params, cap, out, raise_on_pair_failure, seeded=None):
        """System::Tracking for many pairs in one device-resident call (fn: uwt_tracking_batch or uwt_tracking_orb_batch), host in and
        out.  prev: None, or one
        KEYPOINT array per pair (what the previous frame kept; an empty one for a pair that has none), or the packed form
        (kp [P, cap] KEYPOINT, n [P] int32).  out: (poses [P, 7] float32, stats [P] STATS, info [P] TRACKING_INFO, good [P, cap]
        MATCH, kept_prev [P, cap] KEYPOINT, kept_cur [P, cap] KEYPOINT) to be written in place — the rows past a pair's count stay
        as they are.  Returns a dict: status (OK or ERR_PAIR_FAILED), poses, stats, info, and per pair good, kept_prev, kept_cur."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        P = ref.size
        kp = n = None
        if isinstance(prev, tuple):
            kp, n = np.ascontiguousarray(prev[0], KEYPOINT), np.ascontiguousarray(prev[1], np.int32)
        elif prev is not None:
            kin = [np.ascontiguousarray(k, KEYPOINT).reshape(-1) for k in prev]
            kp, n = np.zeros((P, max(cap, 1)), KEYPOINT), np.zeros(P, np.int32)
            for i, k in enumerate(kin):
                kp[i, :len(k)], n[i] = k[:cap], len(k)
        if out is None:
            c = max(cap, 1)
            out = (np.zeros((max(P, 1), 7), np.float32), np.zeros(max(P, 1), STATS), np.zeros(max(P, 1), TRACKING_INFO),
                   np.zeros((max(P, 1), c), MATCH), np.zeros((max(P, 1), c), KEYPOINT), np.zeros((max(P, 1), c), KEYPOINT))
        poses, stats, info, good, kept_prev, kept_cur = out
        tail = ()
        if seeded is not None:
            keep, sp = _host_seeds(seeded[0], P)
            tail = (sp, _sopt(seeded[1]))
        st = fn(self._h, P, _p(ref, C.c_int32), _p(tgt, C.c_int32), _ref(params), cap, kp.ctypes.data if kp is not None else None,
                _p(n, C.c_int32) if n is not None else None, _p(poses, C.c_float), stats.ctypes.data, info.ctypes.data,
                good.ctypes.data, kept_prev.ctypes.data, kept_cur.ctypes.data, *tail)
        self._chk_pairs(st, raise_on_pair_failure)
        cnt = info["n_matches"]
        return dict(status=st, poses=poses[:P], stats=stats[:P], info=info[:P], good=[good[i, :cnt[i]].copy() for i in range(P)],
                    kept_prev=[kept_prev[i, :cnt[i]].copy() for i in range(P)], kept_cur=[kept_cur[i, :cnt[i]].copy() for i in range(P)])

    def tracking_batch_async(self, ref_slots, tgt_slots, io, params=None, cap=2048):
        """tracking_batch without waiting, device in and out (uwt_tracking_batch_async); io: _tracking_batch_async."""
        self._tracking_batch_async(lib().uwt_tracking_batch_async, ref_slots, tgt_slots, io, params, cap)

    def tracking_batch_seeded_async(self, ref_slots, tgt_slots, io, params=None, cap=2048, d_seeds_ptr=None, handoff=None):
        """tracking_batch_async from seeds in device memory (uwt_tracking_batch_seeded_async): d_seeds_ptr None or P x 7 float32 —
        a live loop passes the poses buffer of the call before (another buffer than io's)."""
        self._tracking_batch_async(lib().uwt_tracking_batch_seeded_async, ref_slots, tgt_slots, io, params, cap, (d_seeds_ptr, _sopt(handoff)))

    def tracking_orb_batch_seeded_async(self, ref_slots, tgt_slots, io, params=None, cap=2048, d_seeds_ptr=None, handoff=None):
        """tracking_batch_seeded_async for RobustMatcher(1) (uwt_tracking_orb_batch_seeded_async)."""
        self._tracking_batch_async(lib().uwt_tracking_orb_batch_seeded_async, ref_slots, tgt_slots, io, params, cap, (d_seeds_ptr, _sopt(handoff)))

    def _tracking_batch_async(self, fn, ref_slots, tgt_slots, io, params, cap, tail=()):
        """The same enqueued on the context stream with every input and result in device memory (fn: uwt_tracking_batch_async or
        uwt_tracking_orb_batch_async).  io: a
        dict of device addresses — poses (P x 7 float32), info (P TRACKING_INFO), good (P x cap MATCH), kept_prev, kept_cur (P x cap
        KEYPOINT), n_matches (P int32), optionally stats (P STATS) and prev_kp / n_prev (P x cap KEYPOINT, P int32: kept_cur /
        n_matches of the call before, of ANOTHER set of buffers).  Never waits for the device; sync() to wait."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        rec = TrackingIO(*[io.get(k) or None for k in ("prev_kp", "n_prev", "poses", "stats", "info", "good", "kept_prev", "kept_cur",
                                                        "n_matches")])
        self._chk(fn(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), _ref(params), cap, C.byref(rec), *tail))

    def match_descriptors_device_async(self, n_pairs, dim, cap, d_query_ptr, d_n_query_ptr, d_train_ptr, d_n_train_ptr, d_matches_ptr,
                                       d_counts_ptr, ratio=0.65, norm=NORM_L2):
        """match_descriptors_batch_async with both descriptor sets (P x cap x dim) and their counts (P int32) already in device
        memory, read in place (uwt_match_descriptors_device_async); a device count outside 0..cap is taken as 0.  sync() to wait."""
        self._chk(lib().uwt_match_descriptors_device_async(self._h, n_pairs, norm, dim, d_query_ptr, d_n_query_ptr, d_train_ptr,
                                                           d_n_train_ptr, cap, ratio, d_matches_ptr, d_counts_ptr))

    def surf_integral(self, slot):
        """The integral image of a slot's level-0 plane (uwt_surf_integral): (h + 1) x (w + 1) uint32"""
        out = np.zeros((self.params.height + 1, self.params.width + 1), np.uint32)
        self._chk(lib().uwt_surf_integral(self._h, slot, _p(out, C.c_uint32)))
        return out

    def surf_response_layer(self, slot, octave, layer):
        """One fast-Hessian response layer on its octave's grid (uwt_surf_response_layer): gh x gw float64, NaN where none exists"""
        out = np.zeros(max(1, (self.params.height >> max(octave, 0)) * (self.params.width >> max(octave, 0))), np.float64)
        gw, gh = C.c_int32(0), C.c_int32(0)
        self._chk(lib().uwt_surf_response_layer(self._h, slot, octave, layer, _p(out, C.c_double), C.byref(gw), C.byref(gh)))
        return out[:gw.value * gh.value].reshape(gh.value, gw.value)

    def add_patch_points(self, lvl, pts, patch_size=5, cap=None):
        """Tracker::AddPatchPointsFeatures (src/Tracker.cpp:599-629).  Returns (table, full count)."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        cap = pts.shape[0] * patch_size * patch_size if cap is None else cap
        out = np.empty((max(cap, 1), 4), np.float32)
        cnt = C.c_int32()
        self._chk(lib().uwt_add_patch_points(self._h, lvl, _p(pts, C.c_float), pts.shape[0], patch_size, _p(out, C.c_float), cap,
                                             C.byref(cnt)))
        return out[:min(cnt.value, cap)].copy(), cnt.value

    def residual_jacobian_weighted(self, ref_slot, tgt_slot, lvl, pose):
        pose = np.ascontiguousarray(pose, np.float32)
        L = self.level_info(lvl)
        n = L.w * L.h
        acc = Accum()
        err, inv_mad = C.c_double(), C.c_float()
        J = np.empty((n, 6), np.float32)
        r = np.empty(n, np.float32)
        v = np.empty(n, np.uint8)
        w = np.empty(n, np.float32)
        self._chk(lib().uwt_residual_jacobian_weighted(self._h, ref_slot, tgt_slot, lvl, _p(pose, C.c_float), C.byref(acc),
                                                       C.byref(err), C.byref(inv_mad), _p(J, C.c_float), _p(r, C.c_float),
                                                       _p(v, C.c_uint8), _p(w, C.c_float)))
        return dict(_accum_fields(acc), J=J, r=r, valid=v, w=w, err_num=err.value, inv_mad=inv_mad.value)

    # -- did the alignment work: ObtainImageTransformed / DebugShowWarpedPerspective
    def obtain_image_transformed(self, slot, lvl, pts, warped, image=None):
        """Tracker::ObtainImageTransformed (src/Tracker.cpp:1473-1525) for one explicit table: original = the image plane of `slot` at
        `lvl`, pts / warped: N x 4, image: the output image as it is before the call (img_h x img_w u8; None: zeros).  Returns (the
        output image, validPixel)."""
        L = self.level_info(lvl)
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        warped = np.ascontiguousarray(warped, np.float32).reshape(-1, 4)
        assert pts.shape == warped.shape
        out = np.zeros((L.img_h, L.img_w), np.uint8) if image is None else np.array(image, np.uint8, order="C")
        assert out.shape == (L.img_h, L.img_w)
        valid = np.empty((L.img_h, L.img_w), np.uint8)
        self._chk(lib().uwt_obtain_image_transformed(self._h, slot, lvl, _p(pts, C.c_float), _p(warped, C.c_float), pts.shape[0],
                                                     _p(out, C.c_uint8), _p(valid, C.c_uint8)))
        return out, valid

    def warp_image_batch(self, ref_slots, tgt_slots, poses, lvl=0, absdiff=True, raise_on_pair_failure=False):
        """The dense form for many pairs, host in and out (uwt_warp_image_batch): poses [P, 7].  Returns a dict: status (OK or
        ERR_PAIR_FAILED), warped, valid, absdiff ([P, img_h, img_w] u8; absdiff None when not asked for) and quality ([P] WARP_QUALITY)."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        P = ref.size
        assert tgt.size == P and poses.shape[0] == P
        L = self.level_info(lvl)
        warped = np.zeros((max(P, 1), L.img_h, L.img_w), np.uint8)
        valid = np.zeros_like(warped)
        diff = np.zeros_like(warped) if absdiff else None
        quality = np.zeros(max(P, 1), WARP_QUALITY)
        st = lib().uwt_warp_image_batch(self._h, P, _p(ref, C.c_int32), _p(tgt, C.c_int32), lvl, _p(poses, C.c_float),
                                        _p(warped, C.c_uint8), _p(valid, C.c_uint8), _p(diff, C.c_uint8) if absdiff else None,
                                        quality.ctypes.data)
        self._chk_pairs(st, raise_on_pair_failure)
        return dict(status=st, warped=warped[:P], valid=valid[:P], absdiff=diff[:P] if absdiff else None, quality=quality[:P])

    def warp_image_batch_async(self, ref_slots, tgt_slots, d_poses_ptr, io, lvl=0):
        """The same enqueued on the context stream with the poses and every result in device memory (uwt_warp_image_batch_async).
        d_poses_ptr: P x 7 float32, e.g. the pose buffer of a tracking call enqueued before, with no sync() in between; io: a dict of
        device addresses — quality (P WARP_QUALITY) and optionally warped, valid, absdiff (P x pitch x img_h u8 each).  Never waits
        for the device; sync() to wait."""
        ref, tgt = _pair_lists(ref_slots, tgt_slots)
        rec = WarpImageIO(*[io.get(k) or None for k in ("warped", "valid", "absdiff", "quality")])
        self._chk(lib().uwt_warp_image_batch_async(self._h, ref.size, _p(ref, C.c_int32), _p(tgt, C.c_int32), lvl, d_poses_ptr, C.byref(rec)))

    def warp_mosaic(self, ref_slot, tgt_slot, lvl, warped):
        """The image of Tracker::DebugShowWarpedPerspective (src/Tracker.cpp:1694-1737) for one pair: [image1 | image2] over
        [blend(warped, image2) | blend(image1, image2)], 2 img_h x 2 img_w u8 (uwt_warp_mosaic)."""
        L = self.level_info(lvl)
        warped = np.ascontiguousarray(warped, np.uint8)
        assert warped.shape == (L.img_h, L.img_w)
        out = np.empty((2 * L.img_h, 2 * L.img_w), np.uint8)
        self._chk(lib().uwt_warp_mosaic(self._h, ref_slot, tgt_slot, lvl, _p(warped, C.c_uint8), _p(out, C.c_uint8)))
        return out

    # -- EXTENSION: depth from tracked motion
    def sweep_depth(self, ref_slots, view_slots, poses, codes, params=None, cost=True, outcome=True, raise_on_failure=False):
        """The depth sweep for many jobs, host in and out (uwt_sweep_depth_batch): ref_slots [J], view_slots [J, n_views], poses
        [J, n_views, 7] (X_view = T X_ref), codes [n_hyp] u16.  params: SweepParams (n_views and n_hyp are set from the arrays when
        None).  Returns a dict: status (OK or ERR_PAIR_FAILED), depth, cost ([J, img_h, img_w] u16), outcome ([J, img_h, img_w] u8; cost /
        outcome None when not asked for) and info ([J] SWEEP_INFO)."""
        ref = np.ascontiguousarray(ref_slots, np.int32).reshape(-1)
        J = ref.size
        views = np.ascontiguousarray(view_slots, np.int32).reshape(max(J, 1), -1) if J else np.zeros((0, 1), np.int32)
        codes = np.ascontiguousarray(codes, np.uint16).reshape(-1)
        if params is None:
            params = default_sweep_params(n_views=views.shape[1], n_hyp=codes.size)
        poses = np.ascontiguousarray(poses, np.float32).reshape(-1, 7)
        nl = self.params.n_levels
        L = self.level_info(params.lvl if 0 <= params.lvl < nl else 0)
        shape = (max(J, 1), L.img_h, L.img_w)
        depth = np.zeros(shape, np.uint16)
        cst = np.zeros(shape, np.uint16) if cost else None
        out = np.zeros(shape, np.uint8) if outcome else None
        info = np.zeros(max(J, 1), SWEEP_INFO)
        st = lib().uwt_sweep_depth_batch(self._h, J, _p(ref, C.c_int32), _p(views, C.c_int32), _p(poses, C.c_float), _p(codes, C.c_uint16),
                                         C.byref(params), _p(depth, C.c_uint16), _p(cst, C.c_uint16) if cost else None,
                                         _p(out, C.c_uint8) if outcome else None, info.ctypes.data)
        self._chk_pairs(st, raise_on_failure)
        return dict(status=st, depth=depth[:J], cost=cst[:J] if cost else None, outcome=out[:J] if outcome else None, info=info[:J])

    def sweep_depth_async(self, ref_slots, view_slots, d_poses_ptr, codes, io, params=None):
        """The same enqueued on the context stream with the poses and every result in device memory (uwt_sweep_depth_batch_async).
        d_poses_ptr: J x n_views x 7 float32, e.g. the pose buffer of a tracking call enqueued before, with no sync() in between; io: a
        dict of device addresses — depth (J x pitch x img_h u16; for one job the reference slot's own depth plane is valid), info
        (J SWEEP_INFO) and optionally cost (u16), outcome (u8).  Never waits for the device; sync() to wait."""
        ref = np.ascontiguousarray(ref_slots, np.int32).reshape(-1)
        views = np.ascontiguousarray(view_slots, np.int32).reshape(-1)
        codes = np.ascontiguousarray(codes, np.uint16).reshape(-1)
        if params is None:
            params = default_sweep_params(n_views=views.size // max(ref.size, 1), n_hyp=codes.size)
        rec = SweepIO(*[io.get(k) or None for k in ("depth", "cost", "outcome", "info")])
        self._chk(lib().uwt_sweep_depth_batch_async(self._h, ref.size, _p(ref, C.c_int32), _p(views, C.c_int32), d_poses_ptr,
                                                    _p(codes, C.c_uint16), C.byref(params), C.byref(rec)))

    # -- the map: Visualizer::AddPointCloudFromRGBD
    def point_cloud_batch(self, slots, traj, params=None, cap=None, raise_on_failure=False):
        """The cloud of resident frames, host in and out (uwt_point_cloud_batch): traj [F, 7], the accumulation with reference_axes = 0.
        cap None: room for every selected row.  Returns a dict: status (OK, ERR_PAIR_FAILED or ERR_CAPACITY), points ([written]
        CLOUD_POINT), info ([F] CLOUD_INFO) and call (the call's CLOUD_INFO record: offset = the full count)."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        traj = np.ascontiguousarray(traj, np.float32).reshape(-1, 7)
        F = slots.size
        assert traj.shape[0] == F
        params = default_cloud_params() if params is None else params
        if cap is None:
            L = self.level_info(0)
            cap = F * (-(-(L.w * L.h) // max(int(params.stride), 1)))
        pts = np.zeros(max(cap, 1), CLOUD_POINT)
        info = np.zeros(F + 1, CLOUD_INFO)
        st = lib().uwt_point_cloud_batch(self._h, F, _p(slots, C.c_int32), _p(traj, C.c_float), C.byref(params), pts.ctypes.data, cap,
                                         info.ctypes.data)
        self._chk(st, allow=() if raise_on_failure else (ERR_PAIR_FAILED, ERR_CAPACITY))
        return dict(status=st, points=pts[:int(info[F]["written"])], info=info[:F], call=info[F])

    def point_cloud_batch_async(self, slots, d_traj_ptr, d_points_ptr, cap, d_info_ptr, params=None):
        """The same enqueued on the context stream with the poses and every result in device memory (uwt_point_cloud_batch_async):
        d_traj_ptr F x 7 float32 (e.g. what accumulate_trajectory_device_async left, with no sync() in between), d_points_ptr cap
        CLOUD_POINT records, d_info_ptr F + 1 CLOUD_INFO records.  Never waits for the device; sync() to wait."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        params = default_cloud_params() if params is None else params
        self._chk(lib().uwt_point_cloud_batch_async(self._h, slots.size, _p(slots, C.c_int32), d_traj_ptr, C.byref(params),
                                                    d_points_ptr, cap, d_info_ptr))

    def point_cloud_points(self, slot, pts, traj_pose, params=None, cap=None):
        """Visualizer::AddPointCloudFromRGBD (src/Visualizer.cpp:421-446) on one explicit N x 4 table (uwt_point_cloud_points); `slot`
        serves the intensities.  Returns (points [min(count, cap)] CLOUD_POINT, the full count, status OK or ERR_CAPACITY)."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 4)
        pose = np.ascontiguousarray(traj_pose, np.float32).reshape(7)
        params = default_cloud_params() if params is None else params
        n = pts.shape[0]
        cap = -(-n // max(int(params.stride), 1)) if cap is None else cap
        out = np.zeros(max(cap, 1), CLOUD_POINT)
        cnt = C.c_int64()
        st = lib().uwt_point_cloud_points(self._h, slot, _p(pts, C.c_float), n, _p(pose, C.c_float), C.byref(params),
                                          out.ctypes.data, cap, C.byref(cnt))
        self._chk(st, allow=(ERR_CAPACITY,))
        return out[:min(cnt.value, cap)], cnt.value, st

    def accumulate_trajectory_device_async(self, d_poses_ptr, n, d_traj_ptr, start=None, t_scale=1.0, reference_axes=False):
        """uwt_accumulate_trajectory on device pointers (n x 7 float32 each), enqueued on the context stream: no copy, no wait."""
        start = np.array([0, 0, 0, 1, 0, 0, 0], np.float32) if start is None else np.ascontiguousarray(start, np.float32)
        self._chk(lib().uwt_accumulate_trajectory_device_async(self._h, d_poses_ptr, int(n), _p(start, C.c_float), t_scale,
                                                               int(bool(reference_axes)), d_traj_ptr))

    def accumulate_trajectory_device_from_async(self, d_poses_ptr, n, d_start_ptr, d_traj_ptr, t_scale=1.0, reference_axes=False):
        """The same behind a previous pose in device memory (uwt_accumulate_trajectory_device_from_async): d_start_ptr 7 float32, a row of
        an earlier accumulation made with reference_axes False."""
        self._chk(lib().uwt_accumulate_trajectory_device_from_async(self._h, d_poses_ptr, int(n), d_start_ptr, t_scale,
                                                                    int(bool(reference_axes)), d_traj_ptr))


class Ingest:
    """Frame ingest next to the path: undistortion maps + fused remap/crop into a tracker slot."""

    def __init__(self, K4, dist4, in_w, in_h, out_w, out_h, device=0):
        K = np.ascontiguousarray(K4, np.float32)
        d = np.ascontiguousarray(dist4, np.float32)
        self._h = C.c_void_p()
        nk = np.empty(4, np.float32)
        st = lib().uwt_ingest_create(_p(K, C.c_float), _p(d, C.c_float), in_w, in_h, out_w, out_h, device, C.byref(self._h),
                                     _p(nk, C.c_float))
        if st:
            raise UwtError(st, lib().uwt_status_string(st).decode())
        self.newK = nk
        self.in_w, self.in_h, self.out_w, self.out_h = in_w, in_h, out_w, out_h

    def close(self):
        if self._h:
            lib().uwt_ingest_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st):
        if st:
            raise UwtError(st, lib().uwt_status_string(st).decode())

    def maps(self):
        m1 = np.empty((self.out_h, self.out_w, 2), np.int16)
        m2 = np.empty((self.out_h, self.out_w), np.uint16)
        self._chk(lib().uwt_ingest_maps(self._h, _p(m1, C.c_int16), _p(m2, C.c_uint16)))
        return m1, m2

    def undistort(self, raw):
        raw = np.asarray(raw)
        assert raw.dtype == np.uint8 and raw.shape == (self.in_h, self.in_w) and raw.strides[1] == 1
        out = np.empty((self.out_h, self.out_w), np.uint8)
        self._chk(lib().uwt_ingest_undistort(self._h, _p(raw, C.c_uint8), raw.strides[0], _p(out, C.c_uint8)))
        return out

    def calculate_roi(self, raw_first):
        raw = np.asarray(raw_first)
        roi = np.empty(4, np.int32)
        self._chk(lib().uwt_ingest_calculate_roi(self._h, _p(raw, C.c_uint8), raw.strides[0], _p(roi, C.c_int32)))
        return roi

    def frame(self, ctx, slot, raw, x0, y0):
        raw = np.asarray(raw)
        assert raw.dtype == np.uint8 and raw.shape == (self.in_h, self.in_w) and raw.strides[1] == 1
        self._chk(lib().uwt_ingest_frame(self._h, ctx._h, slot, _p(raw, C.c_uint8), raw.strides[0], x0, y0))
