"""ctypes binding of libht_mi355x.so (the C-ABI declared in include/ht_mi355x.h).

There is no CPU fallback: if the library is missing it is built with hipcc; if it cannot be loaded, or a context cannot be
created on a gfx950 device, an exception is raised.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

HERE = os.path.dirname(os.path.abspath(__file__))
HT_OK = 0
CNN_IN, CNN_OUT, CNNB_COUNT, POSE, STATE, CAM, ANALYSIS = 4096, 2304, 9458400, 7, 13, 12, 84
MAXPTS, ROW, CONTACT = 4096, 16, 12      # HT_MAX_POINTS
LABELS_SEGMENT_FRAME = 1      # HT_LABELS_SEGMENT_FRAME
LABELS_SIDE128 = 2            # HT_LABELS_SIDE128
SENSOR_IVY, SENSOR_DS4 = 0, 1 # HT_SENSOR_IVY, HT_SENSOR_DS4
JOINTS_COM_POSES = 1          # HT_JOINTS_COM_POSES
SAMPLE_ENHANCED = 2           # HT_SAMPLE_ENHANCED
SCENE_RIGHT, SCENE_LEFT, SCENE_ABSENT, SCENE_MAX_HANDS = 0, 1, 255, 4      # HT_SCENE_RIGHT, any value but 0 and 255, HT_SCENE_ABSENT, HT_SCENE_MAX_HANDS
SPLIT_RIGHT_IS_LOW_X, SPLIT_MIRROR_LEFT = 1, 2      # HT_SPLIT_RIGHT_IS_LOW_X, HT_SPLIT_MIRROR_LEFT
SPLIT_MODEL_ALWAYS, SPLIT_MODEL_MERGED, SPLIT_USER_POSES = 0, 1, 4      # HT_SPLIT_MODEL_ALWAYS, HT_SPLIT_MODEL_MERGED, HT_SPLIT_USER_POSES
KP_COM_POSES = 1              # HT_KP_COM_POSES
KP_FEATURE8, KP_SKELETON, KP_CALLER, KP_MAX, KP_MAX_THR = 0, 1, 2, 64, 32      # HT_KP_FEATURE8, HT_KP_SKELETON, HT_KP_CALLER, HT_KP_MAX, HT_KP_MAX_THR
KPFIT_KEEP_MOMENTA = 1        # HT_KPFIT_KEEP_MOMENTA
VIEWS_MAX = 4                 # HT_VIEWS_MAX
CNN128_IN, CNNB128_COUNT = 16384, 30429920
# ht_debug_train_buffers: (name, floats, shape) of the segments of act and err, in order (None: padding)
TRAIN_ACT = (("a1", 57600, (16, 60, 60)), ("a3", 3600, (16, 15, 15)), ("a5", 9216, (64, 12, 12)), ("a6", 2304, (2304,)), ("a8", 2048, (2048,)))
TRAIN_ERR = (("e9", 2304, (2304,)), ("e7", 2048, (2048,)), ("e6", 2304, (2304,)), ("part3", 57600, (16, 3600)), ("sqp", 9, (9,)), (None, 7, None))

# every symbol include/ht_mi355x.h declares (checked by tests/test_abi.py)
SYMBOLS = (
    "ht_create", "ht_destroy", "ht_model_bake", "ht_last_error", "ht_get_params", "ht_set_params", "ht_model_info", "ht_config_read", "ht_scale",
    "ht_cnn_load_weights", "ht_cnn_eval", "ht_cnn_eval_dev", "ht_cnn_load_weights_sized", "ht_cnn_eval_sized", "ht_cnn_eval_sized_dev", "ht_cnn_train", "ht_cnn_get_weights", "ht_expected_cnn", "ht_expected_cnn_full",
    "ht_expected_cnn_batch", "ht_expected_cnn_dev", "ht_cnn_input_dev", "ht_cnn_train_dev", "ht_cnn_train_batch_dev", "ht_cnn_train_batch", "ht_debug_train_batch_buffers",
    "ht_cnn_train_batch_sized_dev", "ht_cnn_train_batch_sized", "ht_cnn_get_weights_sized", "ht_debug_train_batch_buffers_sized", "ht_cnn_input_sized_dev",
    "ht_cnn_grad_batch_sized_dev", "ht_cnn_grad_batch_sized", "ht_cnn_grad_get_sized", "ht_cnn_grad_set_sized", "ht_cnn_grad_ptr_sized", "ht_opt_default", "ht_cnn_opt_step_sized_dev",
    "ht_cnn_opt_reset_sized", "ht_cnn_opt_state_get_sized", "ht_cnn_opt_state_set_sized", "ht_cnn_opt_last_sized", "ht_cnn_train_opt_sized_dev",
    "ht_model_open", "ht_model_close", "ht_model_error", "ht_model_counts", "ht_model_body", "ht_model_body_mesh", "ht_model_body_sdmesh", "ht_model_hitcheck", "ht_model_hitcheck_mesh", "ht_model_render_mesh", "ht_model_scale", "ht_render_mesh_depth", "ht_render_mesh_depth_dev",
    "ht_model_raster_mesh", "ht_raster_mesh_depth", "ht_raster_mesh_depth_dev",
    "ht_model_raster_scene", "ht_raster_scene_depth", "ht_raster_scene_depth_dev",
    "ht_tracker_reset", "ht_get_state", "ht_set_state", "ht_get_tracker_flags", "ht_set_tracker_flags", "ht_update_sync", "ht_update_dev", "ht_update_frames_sync", "ht_update_frames_dev", "ht_update_direct_sync", "ht_update_direct_dev", "ht_update_cnn_model_sync", "ht_get_cnn_results", "ht_get_cnn_layers", "ht_get_cnn_layers_sized", "ht_frames_overflow", "ht_reserve_points", "ht_point_capacity", "ht_capacity_events", "ht_segment_vr", "ht_segment_vr_dev", "ht_segment_vr_supported", "ht_segment_vr_sized", "ht_segment_vr_sized_dev", "ht_update_frames_sized_sync", "ht_update_frames_sized_dev", "ht_render_depth", "ht_render_depth_dev", "ht_slowfit", "ht_set_points", "ht_fit_rows", "ht_physics_update",
    "ht_stage_prepare", "ht_stage_decode", "ht_stage_fit_error", "ht_stage_cloud_rows", "ht_stage_contacts", "ht_stage_fit", "ht_debug_contact_plan",
    "ht_stage_multistep", "ht_stage_multistep_range", "ht_stage_scratch_unibody", "ht_stage_scratch_unibody_listed", "ht_debug_row_counts", "ht_stage_chamber", "ht_profile_enable", "ht_profile_read", "ht_debug_solve_stats", "ht_debug_contact_stats", "ht_debug_solver_build", "ht_debug_reset_flags", "ht_debug_reset_organisation", "ht_update_passes_sync", "ht_job_start", "ht_job_poll", "ht_job_wait", "ht_job_collect", "ht_debug_contact_kernel", "ht_debug_stream_edges", "ht_debug_contact_order", "ht_debug_rank_desc", "ht_contact_capacity", "ht_debug_solve_tables", "ht_debug_solve_tables_header", "ht_debug_train_buffers",
    "ht_sensor_out_dims", "ht_sensor_filter", "ht_sensor_filter_dev", "ht_sensor_background", "ht_sensor_background_dev",
    "ht_sensor_noise_default", "ht_sensor_simulate", "ht_sensor_simulate_dev",
    "ht_model_joint_limits", "ht_joint_coords", "ht_joint_coords_dev", "ht_joint_pose", "ht_joint_pose_dev", "ht_sample_poses", "ht_sample_poses_dev",
    "ht_mirror_frames", "ht_mirror_frames_dev", "ht_mirror_cams", "ht_mirror_cams_dev", "ht_mirror_poses", "ht_mirror_poses_dev", "ht_update_hands_sync", "ht_update_hands_dev", "ht_reserve_hands", "ht_hands_capacity",
    "ht_model_mirror", "ht_model_body_planes",
    "ht_split_hands", "ht_split_hands_dev", "ht_update_two_hands_sync", "ht_update_two_hands_dev",
    "ht_split_hands_model", "ht_split_hands_model_dev", "ht_update_two_hands_model_sync", "ht_update_two_hands_model_dev",
    "ht_keypoint_table", "ht_keypoints", "ht_keypoints_dev", "ht_keypoint_errors", "ht_keypoint_errors_dev", "ht_depth_compare", "ht_depth_compare_dev",
    "ht_pose_depth_residual", "ht_pose_depth_residual_dev", "ht_pose_mesh_residual", "ht_pose_mesh_residual_dev",
    "ht_kpfit_default", "ht_fit_keypoints", "ht_fit_keypoints_dev",
    "ht_views_default", "ht_fuse_views", "ht_fuse_views_dev", "ht_stage_view_rows", "ht_fit_views", "ht_fit_views_dev", "ht_update_views_sync", "ht_update_views_dev", "ht_debug_prepare_frames_dev", "ht_debug_fit_rows_pass_dev",
    "ht_calib_default", "ht_calibrate_view", "ht_calibrate_view_dev",
    "ht_size_default", "ht_estimate_scale", "ht_estimate_scale_dev",
    "ht_comm_available", "ht_comm_unique_id", "ht_comm_init", "ht_comm_info", "ht_gather_poses_dev", "ht_gather_wait", "ht_gather_wait_host", "ht_comm_destroy",
)


class Params(C.Structure):
    _fields_ = [("full_reset_on_error", C.c_float), ("angles_only", C.c_int), ("always_take_cnn", C.c_int), ("drangey", C.c_float), ("boundary_planes", C.c_int),
                ("microforce", C.c_float), ("cloudforce_max_point", C.c_float), ("cloudforce_max_sum", C.c_float), ("mainthreadpasses", C.c_int),
                ("subsample_fraction", C.c_int), ("min_point_num", C.c_int), ("accum_error_threshold", C.c_float), ("min_cray_prob", C.c_float),
                ("steps", C.c_int), ("steps_keypoints", C.c_int), ("steps_keyangles", C.c_int), ("steps_palmangle", C.c_int), ("steps_cloudstart", C.c_int), ("steps_unibody", C.c_int),
                ("physics_iterations", C.c_int), ("physics_iterations_post", C.c_int), ("physics_use_collision", C.c_int),
                ("physics_weak_force", C.c_float), ("bone_sum_error_scale", C.c_float), ("unibody_force", C.c_float),
                ("subsample_voxel", C.c_int), ("subsample_size", C.c_float)]


class SensorNoise(C.Structure):
    """ht_sensor_noise (include/ht_mi355x.h): the noise set of ht_sensor_simulate, field for field."""
    _fields_ = [("seed", C.c_uint64), ("first_index", C.c_uint64), ("far_count", C.c_int), ("sigma0_256", C.c_int), ("sigma2", C.c_int), ("edge_step", C.c_int), ("slope_step", C.c_int),
                ("p_edge_drop", C.c_int), ("p_edge_fly", C.c_int), ("p_slope_drop", C.c_int), ("p_hole", C.c_int), ("fly_bg_count", C.c_int), ("disparity_k", C.c_int), ("wall_count", C.c_int),
                ("ir_floor", C.c_int), ("ir_gain", C.c_int), ("ir_noise", C.c_int)]

    def but(self, **kw):
        """a copy with some fields changed"""
        n = SensorNoise.from_buffer_copy(self)
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("ht_sensor_noise has no field %r" % k)
            setattr(n, k, int(v))
        return n


OPT_SGD, OPT_MOMENTUM, OPT_NESTEROV, OPT_ADAM = 0, 1, 2, 3      # HT_OPT_*
OPT_KINDS = {"sgd": OPT_SGD, "momentum": OPT_MOMENTUM, "nesterov": OPT_NESTEROV, "adam": OPT_ADAM}


class Opt(C.Structure):
    """ht_opt (include/ht_mi355x.h): the optimiser ht_cnn_opt_step_sized_dev applies, field for field.  Opt.default(kind) is ht_opt_default."""
    _fields_ = [("kind", C.c_int), ("lr", C.c_float), ("momentum", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("decoupled_decay", C.c_int), ("grad_scale", C.c_float), ("clip_norm", C.c_float)]

    @classmethod
    def default(cls, kind, **kw):
        """ht_opt_default for a kind (a number or "sgd" / "momentum" / "nesterov" / "adam"), then the fields given"""
        o = cls()
        if load().ht_opt_default(OPT_KINDS.get(kind, -1) if isinstance(kind, str) else int(kind), C.byref(o)) != 0:
            raise ValueError("unknown optimiser kind %r" % (kind,))
        return o.but(**kw)

    def but(self, **kw):
        """a copy with some fields changed"""
        n = Opt.from_buffer_copy(self)
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("ht_opt has no field %r" % k)
            setattr(n, k, v)
        return n


class KpFit(C.Structure):
    """ht_kpfit: the options of ht_fit_keypoints (kpfit_default() fills in slowfit's figures)"""
    _fields_ = [("steps", C.c_int), ("max_force", C.c_float), ("ray_radius", C.c_float), ("ray_force", C.c_float), ("flags", C.c_int)]


class Views(C.Structure):
    """ht_views: the options of ht_fuse_views (Context.views_default() fills in the tracker's figures)"""
    _fields_ = [("range_lo", C.c_float), ("range_hi", C.c_float), ("fraction", C.c_int), ("mirror_eps", C.c_float)]


class Calib(C.Structure):
    """ht_calib: the options of ht_calibrate_view (Context.calib_default() fills in the documented defaults)"""
    _fields_ = [("range_lo", C.c_float), ("range_hi", C.c_float), ("fraction", C.c_int), ("mode", C.c_int), ("iterations", C.c_int), ("max_dist", C.c_float), ("damping", C.c_float),
                ("min_points", C.c_int), ("centre", C.c_float * 3)]


CALIB_RIG, CALIB_PER_SLOT, CALIB_STATS = 0, 1, 27
CALIB_FEW_INLIERS, CALIB_BAD_PIVOT = 1, 2


class Size(C.Structure):
    """ht_size: the options of ht_estimate_scale (Context.size_default() fills in the documented defaults)"""
    _fields_ = [("range_lo", C.c_float), ("range_hi", C.c_float), ("fraction", C.c_int), ("mode", C.c_int), ("free_pose", C.c_int), ("iterations", C.c_int), ("max_dist", C.c_float),
                ("damping", C.c_float), ("min_points", C.c_int), ("scale0", C.c_float), ("scale_lo", C.c_float), ("scale_hi", C.c_float)]


SIZE_SHARED, SIZE_PER_SLOT, SIZE_STATS, SIZE_SLOT_STATS = 0, 1, 6, 3
SIZE_FEW_INLIERS, SIZE_BAD_PIVOT, SIZE_CLAMPED = 1, 2, 4


def size_row(N, B):
    """HT_SIZE_ROW: the float64 values of one row of ht_estimate_scale's stats"""
    return N * SIZE_STATS + B * SIZE_SLOT_STATS


class HTError(RuntimeError):
    pass


_lib = None


def lib_path():
    return _build.LIB


def segment_vr_supported(w, h, side):
    """Whether the sized segmentation and update calls take w x h frames at tile side `side` (ht_segment_vr_supported; no context, no GPU)."""
    return load().ht_segment_vr_supported(int(w), int(h), int(side)) == 0


def load(build_if_missing=True):
    """Load (building first if needed) the shared library; raises if that is impossible."""
    global _lib
    if _lib is not None:
        return _lib
    if build_if_missing and _build.stale():
        _build.build(verbose=False)
    if not os.path.exists(_build.LIB):
        raise HTError("libht_mi355x.so is missing and could not be built; the MI355X path has no fallback")
    L = C.CDLL(_build.LIB)
    fp, ip, vp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.c_void_p
    u16p = C.POINTER(C.c_uint16)
    L.ht_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(vp)]
    L.ht_destroy.argtypes = [vp]
    L.ht_last_error.argtypes = [vp]; L.ht_last_error.restype = C.c_char_p
    L.ht_get_params.argtypes = [vp, C.POINTER(Params)]; L.ht_set_params.argtypes = [vp, C.POINTER(Params)]
    L.ht_model_info.argtypes = [vp, ip, ip, ip]
    L.ht_cnn_load_weights.argtypes = [vp, fp, C.c_size_t]
    L.ht_cnn_eval.argtypes = [vp, fp, fp, C.c_int]
    L.ht_cnn_eval_dev.argtypes = [vp, vp, vp, C.c_int, vp]
    L.ht_cnn_load_weights_sized.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.ht_cnn_eval_sized.argtypes = [vp, C.c_int, fp, fp, C.c_int]
    L.ht_cnn_eval_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
    L.ht_tracker_reset.argtypes = [vp, C.c_int, C.c_int, fp]
    L.ht_get_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp]; L.ht_set_state.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp]
    L.ht_get_tracker_flags.argtypes = [vp, C.c_int, C.c_int, fp, ip]
    L.ht_set_tracker_flags.argtypes = [vp, C.c_int, C.c_int, fp, ip]
    L.ht_update_sync.argtypes = [vp, u16p, fp, C.c_int, fp, fp]
    L.ht_update_dev.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp]
    L.ht_update_frames_sync.argtypes = [vp, u16p, fp, C.c_int, C.c_int, C.c_float, C.c_int, fp, fp]
    L.ht_update_frames_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float, vp, C.c_int, vp, vp]
    L.ht_update_direct_sync.argtypes = [vp, u16p, fp, C.c_int, C.c_int, fp, fp]
    L.ht_update_direct_dev.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.ht_frames_overflow.argtypes = [vp, ip]
    L.ht_reserve_points.argtypes = [vp, C.c_int]
    L.ht_point_capacity.argtypes = [vp, ip]
    L.ht_update_cnn_model_sync.argtypes = [vp, u16p, fp, C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, fp, ip, fp]
    L.ht_get_cnn_results.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp]
    L.ht_capacity_events.argtypes = [vp, ip, ip, ip]
    L.ht_stage_prepare.argtypes = [vp, u16p, fp, C.c_int, fp, fp, ip]
    L.ht_stage_decode.argtypes = [vp, fp, fp, C.c_int, fp]
    L.ht_stage_fit_error.argtypes = [vp, C.c_int, C.c_int, fp]
    L.ht_stage_cloud_rows.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, fp, ip]
    L.ht_stage_contacts.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, ip]
    L.ht_stage_fit.argtypes = [vp, C.c_int]
    L.ht_stage_multistep.argtypes = [vp, fp, C.c_int]
    L.ht_stage_multistep_range.argtypes = [vp, fp, C.c_int, C.c_int, C.c_int]
    L.ht_stage_scratch_unibody.argtypes = [vp, fp, C.c_int, C.c_int]
    L.ht_debug_row_counts.argtypes = [vp, C.c_int, C.POINTER(C.c_int)]
    L.ht_stage_scratch_unibody_listed.argtypes = [vp, fp, C.c_int, C.c_int, C.POINTER(C.c_int), C.c_int, C.c_int]
    L.ht_profile_enable.argtypes = [vp, C.c_int]
    L.ht_scale.argtypes = [vp, C.c_float]
    L.ht_cnn_train.argtypes = [vp, fp, fp, C.c_int, C.c_float, fp]
    L.ht_cnn_get_weights.argtypes = [vp, fp, C.c_size_t]
    L.ht_debug_train_buffers.argtypes = [vp, fp, C.c_size_t, fp, C.c_size_t]
    L.ht_expected_cnn.argtypes = [fp, fp, fp]
    L.ht_expected_cnn_batch.argtypes = [vp, fp, fp, C.c_int, C.c_int, fp, fp, fp]
    L.ht_expected_cnn_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.ht_cnn_input_dev.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.ht_cnn_train_dev.argtypes = [vp, vp, vp, C.c_int, ip, C.c_int, C.c_float, vp, vp]
    L.ht_cnn_train_batch_dev.argtypes = [vp, vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_float, vp, vp]
    L.ht_cnn_train_batch.argtypes = [vp, fp, fp, C.c_int, C.c_int, C.c_float, fp]
    L.ht_debug_train_batch_buffers.argtypes = [vp, C.c_int] + [fp] * 7
    L.ht_cnn_train_batch_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_float, vp, vp]
    L.ht_cnn_train_batch_sized.argtypes = [vp, C.c_int, fp, fp, C.c_int, C.c_int, C.c_float, fp]
    L.ht_cnn_get_weights_sized.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.ht_debug_train_batch_buffers_sized.argtypes = [vp, C.c_int, C.c_int] + [fp] * 7
    L.ht_cnn_grad_batch_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip, C.c_int, C.c_int, vp, vp]
    L.ht_cnn_grad_batch_sized.argtypes = [vp, C.c_int, fp, fp, C.c_int, C.c_int, fp]
    L.ht_cnn_grad_get_sized.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.ht_cnn_grad_set_sized.argtypes = [vp, C.c_int, fp, C.c_size_t]
    L.ht_cnn_grad_ptr_sized.argtypes = [vp, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.ht_opt_default.argtypes = [C.c_int, C.POINTER(Opt)]
    L.ht_cnn_opt_step_sized_dev.argtypes = [vp, C.c_int, C.POINTER(Opt), vp]
    L.ht_cnn_opt_reset_sized.argtypes = [vp, C.c_int]
    L.ht_cnn_opt_state_get_sized.argtypes = [vp, C.c_int, fp, fp, C.c_size_t, ip]
    L.ht_cnn_opt_state_set_sized.argtypes = [vp, C.c_int, fp, fp, C.c_size_t, C.c_int]
    L.ht_cnn_opt_last_sized.argtypes = [vp, C.c_int, C.POINTER(C.c_double), fp]
    L.ht_cnn_train_opt_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, ip, C.c_int, C.c_int, C.c_int, C.POINTER(Opt), vp, vp]
    L.ht_cnn_input_sized_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.ht_set_points.argtypes = [vp, C.c_int, fp, C.c_int, ip]
    L.ht_slowfit.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int, C.c_int, fp, fp, fp, C.c_int]
    L.ht_get_cnn_layers.argtypes = [vp, C.c_int, C.c_int, fp, fp, fp, fp]
    L.ht_get_cnn_layers_sized.argtypes = [vp, C.c_int, C.c_int, C.c_int, fp, fp, fp, fp]
    L.ht_stage_chamber.argtypes = [vp, C.c_int, C.c_int, fp, ip]
    L.ht_fit_rows.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int, ip, fp, C.c_int, ip, fp, C.c_int, ip, C.c_float]
    L.ht_physics_update.argtypes = [vp, C.c_int, C.c_int, fp, C.c_int, ip, fp, C.c_int, ip]
    L.ht_segment_vr.argtypes = [vp, C.POINTER(C.c_uint16), fp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.POINTER(C.c_uint16), fp]
    L.ht_segment_vr_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, vp, vp, vp]
    L.ht_segment_vr_supported.argtypes = [C.c_int, C.c_int, C.c_int]
    L.ht_segment_vr_sized.argtypes = [vp, C.c_int] + L.ht_segment_vr.argtypes[1:]
    L.ht_segment_vr_sized_dev.argtypes = [vp, C.c_int] + L.ht_segment_vr_dev.argtypes[1:]
    L.ht_update_frames_sized_sync.argtypes = [vp, C.c_int] + L.ht_update_frames_sync.argtypes[1:]
    L.ht_update_frames_sized_dev.argtypes = [vp, C.c_int] + L.ht_update_frames_dev.argtypes[1:]
    L.ht_render_depth.argtypes =[vp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_int, u16p, C.POINTER(C.c_int8)]
    L.ht_render_depth_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_int, vp, vp, vp]
    L.ht_sensor_out_dims.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, ip, ip]
    L.ht_sensor_filter.argtypes = [vp, C.c_int, u16p, C.POINTER(C.c_uint8), fp, C.c_int, C.c_int, C.c_int, C.c_int, u16p, u16p, fp]
    L.ht_sensor_filter_dev.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp, vp, vp]
    L.ht_sensor_background.argtypes = [vp, u16p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, u16p]
    L.ht_sensor_background_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp, vp]
    L.ht_sensor_noise_default.argtypes = [C.c_int, C.c_float, C.c_float, C.POINTER(SensorNoise)]
    L.ht_sensor_simulate.argtypes = [vp, C.c_int, u16p, C.c_int, C.c_int, C.c_int, C.POINTER(SensorNoise), u16p, C.POINTER(C.c_uint8)]
    L.ht_sensor_simulate_dev.argtypes = [vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.POINTER(SensorNoise), vp, vp, vp]
    L.ht_render_mesh_depth.argtypes = [vp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, u16p, C.POINTER(C.c_int8)]
    L.ht_render_mesh_depth_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp]
    L.ht_model_hitcheck_mesh.argtypes = [vp, fp, fp, fp, fp, fp, ip, ip]
    L.ht_model_render_mesh.argtypes = [vp, fp, fp, C.c_int, C.c_int, C.c_float, C.c_float, u16p, C.POINTER(C.c_int8)]
    L.ht_raster_mesh_depth.argtypes = L.ht_render_mesh_depth.argtypes
    L.ht_raster_mesh_depth_dev.argtypes = L.ht_render_mesh_depth_dev.argtypes
    L.ht_model_raster_mesh.argtypes = L.ht_model_render_mesh.argtypes
    i8p, i32p_ = C.POINTER(C.c_int8), C.POINTER(C.c_int32)
    L.ht_model_raster_scene.argtypes = [vp, fp, C.POINTER(C.c_uint8), C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_float, u16p, u16p, i8p, i8p, i32p_]
    L.ht_raster_scene_depth.argtypes = [vp, fp, C.POINTER(C.c_uint8), C.c_int, fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, u16p, u16p, i8p, i8p, i32p_]
    L.ht_raster_scene_depth_dev.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ht_model_scale.argtypes = [vp, C.c_float]
    L.ht_profile_read.argtypes = [vp, C.c_int, C.c_int, C.c_char_p, C.c_int, fp, ip, ip]
    L.ht_debug_solve_stats.argtypes = [vp, C.c_int, fp, C.c_int]
    L.ht_debug_solver_build.argtypes = [vp, C.c_int]
    L.ht_debug_reset_organisation.argtypes = [vp, ip]
    L.ht_debug_reset_flags.argtypes = [vp, ip, C.c_int]
    L.ht_debug_contact_kernel.argtypes = [vp, C.c_int]
    L.ht_debug_stream_edges.argtypes = [vp, C.c_int]
    L.ht_debug_contact_plan.argtypes = [vp, C.c_int, ip, ip]
    L.ht_debug_contact_order.argtypes = [vp, ip, C.c_int, C.c_int, C.c_int, ip]
    L.ht_debug_rank_desc.argtypes = [vp, ip, C.c_int, ip]
    L.ht_debug_solve_tables.argtypes = [vp, C.c_int]
    L.ht_contact_capacity.argtypes = [vp, ip, ip, ip, ip]
    L.ht_debug_solve_tables_header.argtypes = [vp, C.c_int, ip]
    L.ht_comm_unique_id.argtypes = [vp]
    L.ht_comm_init.argtypes = [vp, C.c_int, C.c_int, vp]
    L.ht_comm_info.argtypes = [vp, ip, ip]
    L.ht_gather_poses_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp]
    L.ht_gather_wait.argtypes = [vp, C.c_int, vp]
    L.ht_gather_wait_host.argtypes = [vp, C.c_int]
    L.ht_comm_available.argtypes = []
    L.ht_comm_destroy.argtypes = [vp]
    L.ht_debug_contact_stats.argtypes = [vp, C.c_int, fp, C.c_int]
    L.ht_model_joint_limits.argtypes = [vp, fp, fp, ip]
    L.ht_joint_coords.argtypes = [vp, fp, C.c_int, C.c_int, fp, fp]
    L.ht_joint_coords_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.ht_joint_pose.argtypes = [vp, fp, fp, C.c_int, C.c_int, fp]
    L.ht_joint_pose_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, vp, vp]
    L.ht_sample_poses.argtypes = [vp, fp, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_int, fp, fp]
    L.ht_sample_poses_dev.argtypes = [vp, vp, C.c_int, C.c_uint64, C.c_uint64, C.c_float, C.c_int, vp, vp, vp]
    u8p = C.POINTER(C.c_uint8)
    L.ht_mirror_frames.argtypes = [vp, u16p, C.c_int, C.c_int, C.c_int, u8p, u16p]
    L.ht_mirror_frames_dev.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, vp, vp, vp]
    L.ht_mirror_cams.argtypes = [vp, fp, C.c_int, C.c_int, u8p, fp]
    L.ht_mirror_cams_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.ht_mirror_poses.argtypes = [vp, fp, C.c_int, C.c_int, u8p, fp]
    L.ht_mirror_poses_dev.argtypes = [vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.ht_update_hands_sync.argtypes = [vp, C.c_int, u16p, fp, C.c_int, C.c_int, C.c_float, u8p, C.c_int, fp, fp]
    L.ht_update_hands_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, vp, vp, C.c_int, vp, vp]
    L.ht_reserve_hands.argtypes = [vp, C.c_int, C.c_int]
    L.ht_hands_capacity.argtypes = [vp, C.POINTER(C.c_size_t)]
    L.ht_model_mirror.argtypes = [vp]
    u16, i32p = C.c_uint16, C.POINTER(C.c_int32)
    L.ht_split_hands.argtypes = [vp, u16p, fp, C.c_int, C.c_int, C.c_int, u16, u16, u16, C.c_int, u16, C.c_int, u16p, fp, i32p, i32p, u16p]
    L.ht_split_hands_dev.argtypes = [vp, vp, vp, C.c_int, C.c_int, C.c_int, u16, u16, u16, C.c_int, u16, C.c_int, vp, vp, vp, vp, vp, vp]
    L.ht_update_two_hands_sync.argtypes = [vp, C.c_int, u16p, fp, C.c_int, C.c_int, C.c_float, u16, u16, u16, C.c_int, u16, C.c_int, C.c_int, fp, i32p, fp]
    L.ht_update_two_hands_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, u16, u16, u16, C.c_int, u16, C.c_int, vp, C.c_int, vp, vp, vp]
    L.ht_split_hands_model.argtypes = [vp, u16p, fp, fp, C.c_int, C.c_int, C.c_int, u16, u16, u16, C.c_int, u16, C.c_float, C.c_int, C.c_int, u16p, fp, i32p, i32p, i32p, fp, u16p]
    L.ht_split_hands_model_dev.argtypes = [vp, vp, vp, vp, C.c_int, C.c_int, C.c_int, u16, u16, u16, C.c_int, u16, C.c_float, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.ht_update_two_hands_model_sync.argtypes = [vp, C.c_int, u16p, fp, C.c_int, C.c_int, C.c_float, u16, u16, u16, C.c_int, u16, C.c_float, C.c_int, C.c_int, C.c_int, fp, i32p, i32p, fp]
    L.ht_update_two_hands_model_dev.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int, C.c_float, u16, u16, u16, C.c_int, u16, C.c_float, C.c_int, C.c_int, vp, C.c_int, vp, vp, vp, vp]
    L.ht_model_body_planes.argtypes = [vp, C.c_int, fp, fp]
    dp, i64p, ci, cf = C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int, C.c_float
    L.ht_keypoint_table.argtypes = [vp, ci, ip, ip, fp, ip]
    L.ht_keypoints.argtypes = [vp, fp, ci, ci, ci, ci, ip, fp, ip, u8p, fp, u16p, ci, ci, cf, cf, fp, fp, fp, u8p]
    L.ht_keypoints_dev.argtypes = [vp, vp, ci, ci, ci, ci, ip, fp, ip, vp, vp, vp, ci, ci, cf, cf, vp, vp, vp, vp, vp]
    L.ht_kpfit_default.argtypes = [C.POINTER(KpFit)]
    L.ht_fit_keypoints.argtypes = [vp, ci, ci, ci, ci, ip, fp, ip, ip, fp, fp, fp, fp, C.POINTER(KpFit), fp, fp]
    L.ht_fit_keypoints_dev.argtypes = [vp, ci, ci, ci, ci, ip, fp, ip, ip, vp, vp, vp, vp, C.POINTER(KpFit), vp, vp, vp]
    vwp = C.POINTER(Views)
    L.ht_views_default.argtypes = [vp, vwp]
    L.ht_fuse_views.argtypes = [vp, u16p, fp, fp, ci, ci, ci, ci, vwp, fp, ci, ip, ip, fp, ip]
    L.ht_fuse_views_dev.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vwp, vp, vp, vp, vp, vp]
    L.ht_stage_view_rows.argtypes = [vp, ci, ci, fp, ci, ip]
    L.ht_fit_views.argtypes = [vp, ci, ci, ci, fp]
    L.ht_fit_views_dev.argtypes = [vp, ci, ci, ci, vp, vp]
    L.ht_update_views_sync.argtypes = [vp, ci, u16p, fp, fp, ci, ci, ci, cf, ci, vwp, ci, fp, fp]
    L.ht_update_views_dev.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, cf, vp, ci, vwp, ci, vp, vp]
    L.ht_debug_prepare_frames_dev.argtypes = [vp, vp, vp, ci, ci, ci, vp]
    cbp = C.POINTER(Calib)
    L.ht_calib_default.argtypes = [vp, cbp]
    L.ht_calibrate_view.argtypes = [vp, ci, fp, u16p, fp, ci, ci, ci, cbp, fp, dp]
    L.ht_calibrate_view_dev.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, cbp, vp, vp, vp]
    szp = C.POINTER(Size)
    L.ht_size_default.argtypes = [vp, szp]
    L.ht_estimate_scale.argtypes = [vp, ci, fp, u16p, fp, ci, ci, ci, szp, fp, fp, dp]
    L.ht_estimate_scale_dev.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, szp, vp, vp, vp, vp]
    L.ht_debug_fit_rows_pass_dev.argtypes = [vp, ci, ci, vp]
    L.ht_keypoint_errors.argtypes = [vp, fp, fp, ci, ci, fp, ci, fp, fp, dp, i64p, i64p]
    L.ht_keypoint_errors_dev.argtypes = [vp, vp, vp, ci, ci, fp, ci, vp, vp, vp, vp, vp, vp]
    L.ht_depth_compare.argtypes = [vp, u16p, u16p, ci, ci, ci, ci, ci, ci, i64p]
    L.ht_depth_compare_dev.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, vp]
    L.ht_pose_depth_residual.argtypes = [vp, fp, fp, u16p, ci, ci, ci, ci, cf, ci, ci, ci, i64p, u16p]
    L.ht_pose_depth_residual_dev.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, cf, ci, ci, ci, vp, vp, vp]
    L.ht_pose_mesh_residual.argtypes = L.ht_pose_depth_residual.argtypes
    L.ht_pose_mesh_residual_dev.argtypes = L.ht_pose_depth_residual_dev.argtypes
    for name in SYMBOLS:
        if name not in ("ht_last_error", "ht_model_error"):
            getattr(L, name).restype = C.c_int
    _lib = L
    return L


def model_bake(json_path, out_path, hand_tweaks=True):
    """Host-only model build (PhysModel ctor + LoadHandModel, physmodel.h:444-475, handtrack.h:347-366) -> baked container."""
    r = load().ht_model_bake(str(json_path).encode(), str(out_path).encode(), 1 if hand_tweaks else 0)
    if r != 0:
        raise HTError("ht_model_bake(%s) failed with status %d" % (json_path, r))
    return out_path


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _c(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a


class Context:
    """One (GPU, stream) context = the batched counterpart of a HandTracker object (handtrack.h:513-846)."""

    def __init__(self, model_path, max_batch, device=0):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.ht_create(None if model_path is None else os.fsencode(model_path), int(max_batch), int(device), C.byref(self.h))      # None: a context that serves the net only (ht_mi355x.h)
        if rc != HT_OK:
            msg = self.L.ht_last_error(self.h).decode() if self.h else "ht_create failed"
            if self.h:
                self.L.ht_destroy(self.h)
                self.h = C.c_void_p()
            raise HTError("ht_create: %s (status %d)" % (msg, rc))
        nb, nj, mb = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.ht_model_info(self.h, C.byref(nb), C.byref(nj), C.byref(mb)))
        self.nb, self.nj, self.max_batch = nb.value, nj.value, mb.value

    def close(self):
        if self.h:
            self.L.ht_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != HT_OK:
            raise HTError("%s (status %d)" % (self.L.ht_last_error(self.h).decode(), rc))

    # -- parameters
    @property
    def params(self):
        p = Params()
        self._chk(self.L.ht_get_params(self.h, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.params
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(k)
            setattr(p, k, v)
        self._chk(self.L.ht_set_params(self.h, C.byref(p)))

    # -- CNN
    def load_weights(self, w, side=64):
        """The weights of the net of a side x side input (64: the reference's; 128: BASELINE configs[4]) in .cnnb order."""
        w = _c(w, np.float32); side = self._side(side)
        self._chk(self.L.ht_cnn_load_weights(self.h, _f(w), w.size) if side == 64 else self.L.ht_cnn_load_weights_sized(self.h, side, _f(w), w.size))

    def cnn_eval(self, x, side=64):
        side = self._side(side)
        x = _c(x, np.float32).reshape(-1, side * side)
        out = np.empty((x.shape[0], CNN_OUT), np.float32)
        self._chk(self.L.ht_cnn_eval(self.h, _f(x), _f(out), x.shape[0]) if side == 64 else self.L.ht_cnn_eval_sized(self.h, side, _f(x), _f(out), x.shape[0]))
        return out

    def cnn_eval_dev(self, d_in, d_out, B, stream, side=64):
        side = self._side(side)
        self._chk(self.L.ht_cnn_eval_dev(self.h, d_in, d_out, B, stream) if side == 64 else self.L.ht_cnn_eval_sized_dev(self.h, side, d_in, d_out, B, stream))

    def load_weights128(self, w):
        self.load_weights(w, side=128)

    def cnn128_eval(self, x):
        return self.cnn_eval(x, side=128)

    def cnn128_eval_dev(self, d_in, d_out, B, stream):
        self.cnn_eval_dev(d_in, d_out, B, stream, side=128)

    # -- tracker
    def tracker_reset(self, poses, first=0):
        poses = _c(poses, np.float32).reshape(-1, self.nb, POSE)
        self._chk(self.L.ht_tracker_reset(self.h, first, poses.shape[0], _f(poses)))

    def get_state(self, which, n, first=0):
        s = np.empty((n, self.nb, STATE), np.float32)
        self._chk(self.L.ht_get_state(self.h, which, first, n, _f(s)))
        return s

    def set_state(self, which, state, first=0):
        state = _c(state, np.float32).reshape(-1, self.nb, STATE)
        self._chk(self.L.ht_set_state(self.h, which, first, state.shape[0], _f(state)))

    def tracker_flags(self, n, first=0):
        e = np.empty(n, np.float32); i = np.empty(n, np.int32)
        self._chk(self.L.ht_get_tracker_flags(self.h, first, n, _f(e), _i(i)))
        return e, i

    def set_tracker_flags(self, prev_frame_error, initializing, first=0):
        e = _c(prev_frame_error, np.float32); i = _c(initializing, np.int32)
        self._chk(self.L.ht_set_tracker_flags(self.h, first, e.size, _f(e), _i(i)))

    def _update_io(self, depth, cams, want_cnn, pixels=None, per_frame=1, cam_rows=0):
        """What every update_*_sync starts with -> (B, h, w, depth pointer, cams pointer, poses, cnn, poses pointer, cnn pointer or None): depth as contiguous uint16
        [B,h,w] (pixels: flattened frames [B,pixels]; h and w are None then), cams as float32 (cam_rows: 0 one row per frame, -1 any number of rows, None taken as they
        come), fresh poses [B,nb,7] (per_frame 2: [B,2,nb,7]) and, on request, cnn_out of per_frame * B rows.  The pointers keep their arrays alive."""
        depth = _c(depth, np.uint16)
        if pixels is not None:
            depth = depth.reshape(-1, pixels)
        B, h, w = depth.shape if pixels is None else (depth.shape[0], None, None)
        cams = _c(cams, np.float32)
        if cam_rows is not None:
            cams = cams.reshape(cam_rows or B, CAM)
        poses = np.empty((B, self.nb, POSE) if per_frame == 1 else (B, per_frame, self.nb, POSE), np.float32)
        cnn = np.empty((per_frame * B, CNN_OUT), np.float32) if want_cnn else None
        return B, h, w, depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), poses, cnn, _f(poses), _f(cnn) if want_cnn else None

    def update_sync(self, depth, cams, want_cnn=False):
        B, _, _, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn, pixels=4096, cam_rows=-1)
        self._chk(self.L.ht_update_sync(self.h, dp, cp, B, pp, np_))
        return (poses, cnn) if want_cnn else poses

    def update_dev(self, d_depth, d_cams, d_start, B, d_poses_out, stream):
        self._chk(self.L.ht_update_dev(self.h, d_depth, d_cams, d_start, B, d_poses_out, stream))

    def update_frames_sync(self, depth, cams, segment_scale=0.17, want_cnn=False):
        """HandTracker::update on frames of any size (handtrack.h:693-785): depth u16[B,h,w], cams [B,12] = the frames' cameras."""
        B, h, w, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn)
        self._chk(self.L.ht_update_frames_sync(self.h, dp, cp, w, h, float(segment_scale), B, pp, np_))
        return (poses, cnn) if want_cnn else poses

    def update_frames_dev(self, d_depth, d_cams, w, h, segment_scale, d_start, B, d_poses_out, stream):
        self._chk(self.L.ht_update_frames_dev(self.h, d_depth, d_cams, int(w), int(h), float(segment_scale), d_start, B, d_poses_out, stream))

    def update_frames_sized_sync(self, depth, cams, side=128, segment_scale=0.17, want_cnn=False):
        """HandTracker::update on frames up to 640x480 with the segment cut at `side` for the net of that input size (ht_update_frames_sized_sync): depth u16[B,h,w], cams [B,12]."""
        B, h, w, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn)
        self._chk(self.L.ht_update_frames_sized_sync(self.h, int(side), dp, cp, w, h, float(segment_scale), B, pp, np_))
        return (poses, cnn) if want_cnn else poses

    def update_frames_sized_dev(self, side, d_depth, d_cams, w, h, segment_scale, d_start, B, d_poses_out, stream):
        self._chk(self.L.ht_update_frames_sized_dev(self.h, int(side), d_depth, d_cams, int(w), int(h), float(segment_scale), d_start, B, d_poses_out, stream))

    # ---- left hands (include/ht_mi355x.h "left hands"): hands uint8[B], nonzero = left
    @staticmethod
    def _hands(hands, B):
        if hands is None:
            return None, None
        hands = np.ascontiguousarray(hands, np.uint8).reshape(-1)
        if hands.shape[0] != B:
            raise HTError("hands: one flag per frame")
        return hands, hands.ctypes.data_as(C.POINTER(C.c_uint8))

    def mirror_frames(self, depth, hands=None):
        """depth u16[B,h,w] -> the frames flipped left to right where hands is set (None: everywhere), copied elsewhere (ht_mirror_frames)."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        hands, hp = self._hands(hands, B)
        out = np.empty_like(depth)
        u16 = C.POINTER(C.c_uint16)
        self._chk(self.L.ht_mirror_frames(self.h, depth.ctypes.data_as(u16), w, h, B, hp, out.ctypes.data_as(u16)))
        return out

    def mirror_frames_dev(self, d_depth, w, h, B, d_hands, d_depth_out, stream=None):
        self._chk(self.L.ht_mirror_frames_dev(self.h, d_depth, int(w), int(h), int(B), d_hands, d_depth_out, stream))

    def mirror_cams(self, cams, w, hands=None):
        """cams [B,12] of frames w pixels wide -> the mirrored cameras (cx' = (w-1) - cx, the pose mirrored) where hands is set (ht_mirror_cams)."""
        cams = _c(cams, np.float32); B = cams.shape[0]
        hands, hp = self._hands(hands, B)
        out = np.empty_like(cams)
        self._chk(self.L.ht_mirror_cams(self.h, _f(cams), int(w), B, hp, _f(out)))
        return out

    def mirror_cams_dev(self, d_cams, w, B, d_hands, d_cams_out, stream=None):
        self._chk(self.L.ht_mirror_cams_dev(self.h, d_cams, int(w), int(B), d_hands, d_cams_out, stream))

    def mirror_poses(self, poses, hands=None):
        """poses [B,n,7] (or [B,7]) -> (-px,py,pz, qx,-qy,-qz,qw) where hands is set (ht_mirror_poses)."""
        poses = _c(poses, np.float32); B = poses.shape[0]; per = int(np.prod(poses.shape[1:-1])) if poses.ndim > 2 else 1
        hands, hp = self._hands(hands, B)
        out = np.empty_like(poses)
        self._chk(self.L.ht_mirror_poses(self.h, _f(poses), per, B, hp, _f(out)))
        return out

    def mirror_poses_dev(self, d_poses, per_frame, B, d_hands, d_poses_out, stream=None):
        self._chk(self.L.ht_mirror_poses_dev(self.h, d_poses, int(per_frame), int(B), d_hands, d_poses_out, stream))

    def update_hands_sync(self, depth, cams, hands, side=64, segment_scale=0.17, want_cnn=False):
        """ht_update_frames_sized_sync with a handedness flag per frame (ht_update_hands_sync): the poses of flagged frames are a left hand's; cnn_out stays canonical."""
        B, h, w, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn, cam_rows=None)
        hands, hp = self._hands(hands, B)
        self._chk(self.L.ht_update_hands_sync(self.h, int(side), dp, cp, w, h, float(segment_scale), hp, B, pp, np_))
        return (poses, cnn) if want_cnn else poses

    def update_hands_dev(self, side, d_depth, d_cams, w, h, segment_scale, d_hands, d_start, B, d_poses_out, stream=None):
        self._chk(self.L.ht_update_hands_dev(self.h, int(side), d_depth, d_cams, int(w), int(h), float(segment_scale), d_hands, d_start, int(B), d_poses_out, stream))

    def reserve_hands(self, w, h):
        self._chk(self.L.ht_reserve_hands(self.h, int(w), int(h)))

    def hands_capacity(self):
        """pixels per frame the left-hand staging holds (0: not allocated)"""
        n = C.c_size_t()
        self._chk(self.L.ht_hands_capacity(self.h, C.byref(n)))
        return n.value

    # ---- two hands in one frame (include/ht_mi355x.h "two hands in one frame")
    def split_hands(self, depth, range_lo, range_hi, far, cams=None, max_step=65535, min_pixels=1, flags=0, want_labels=False, want_n=True):
        """depth u16[B,h,w] -> dict(frames u16[B,2,h,w] (0 right, 1 left), info i32[B,2,8], and on request cams [B,2,12], n_components [B], labels u16[B,h/4,w/4]) (ht_split_hands)"""
        depth = _c(depth, np.uint16)
        B, h, w = depth.shape
        u16 = C.POINTER(C.c_uint16); i32 = C.POINTER(C.c_int32)
        out = dict(frames=np.empty((B, 2, h, w), np.uint16), info=np.empty((B, 2, 8), np.int32))
        if cams is not None:
            cams = _c(cams, np.float32); out["cams"] = np.empty((B, 2, CAM), np.float32)
        if want_n:
            out["n_components"] = np.empty(B, np.int32)
        if want_labels:
            out["labels"] = np.empty((B, h // 4, w // 4), np.uint16)
        self._chk(self.L.ht_split_hands(self.h, depth.ctypes.data_as(u16), None if cams is None else _f(cams), w, h, B, int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far), int(flags),
                                        out["frames"].ctypes.data_as(u16), None if cams is None else _f(out["cams"]), out["info"].ctypes.data_as(i32),
                                        out["n_components"].ctypes.data_as(i32) if want_n else None, out["labels"].ctypes.data_as(u16) if want_labels else None))
        return out

    def split_hands_dev(self, d_depth, d_cams, w, h, B, range_lo, range_hi, max_step, min_pixels, far, flags, d_depth_out, d_cams_out, d_info, d_n_components=None, d_labels=None, stream=None):
        self._chk(self.L.ht_split_hands_dev(self.h, d_depth, d_cams, int(w), int(h), int(B), int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far), int(flags), d_depth_out, d_cams_out,
                                            d_info, d_n_components, d_labels, stream))

    def update_two_hands_sync(self, depth, cams, range_lo, range_hi, far, side=64, segment_scale=0.17, max_step=65535, min_pixels=1, flags=0, want_cnn=False):
        """B frames of two hands each in slots 2i (right) and 2i+1 (left): poses [B,2,nb,7] in the camera's space, info i32[B,2,8], and cnn_out [2B,2304] (canonical) on request"""
        B, h, w, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn, per_frame=2, cam_rows=None)
        info = np.empty((B, 2, 8), np.int32)
        self._chk(self.L.ht_update_two_hands_sync(self.h, int(side), dp, cp, w, h, float(segment_scale), int(range_lo), int(range_hi), int(max_step),
                                                  int(min_pixels), int(far), int(flags), B, pp, info.ctypes.data_as(C.POINTER(C.c_int32)), np_))
        return (poses, info, cnn) if want_cnn else (poses, info)

    def update_two_hands_dev(self, side, d_depth, d_cams, w, h, segment_scale, range_lo, range_hi, max_step, min_pixels, far, flags, d_start, B, d_poses_out, d_info=None, stream=None):
        self._chk(self.L.ht_update_two_hands_dev(self.h, int(side), d_depth, d_cams, int(w), int(h), float(segment_scale), int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far), int(flags),
                                                 d_start, int(B), d_poses_out, d_info, stream))

    # ---- two hands that touch or cross (include/ht_mi355x.h "two hands that touch or cross")
    def split_hands_model(self, depth, cams, poses, range_lo, range_hi, far, max_dist=float("inf"), mode=SPLIT_MODEL_ALWAYS, max_step=65535, min_pixels=1, flags=0, want_cams=True, want_n=True, want_source=True,
                          want_dist=False, want_labels=False):
        """depth u16[B,h,w], cams [B,12], poses [B,2,nb,7] (0 right, 1 left, real space) -> dict(frames u16[B,2,h,w], info i32[B,2,8], and on request cams [B,2,12], n_components [B],
        source i32[B], dist f32[B,h/4,w/4,2], labels u16[B,h/4,w/4]) (ht_split_hands_model)"""
        depth = _c(depth, np.uint16); cams = _c(cams, np.float32); poses = _c(poses, np.float32)
        B, h, w = depth.shape
        assert cams.size == B * CAM and (self.nb == 0 or poses.size == B * 2 * self.nb * POSE)
        u16 = C.POINTER(C.c_uint16); i32 = C.POINTER(C.c_int32)
        out = dict(frames=np.empty((B, 2, h, w), np.uint16), info=np.empty((B, 2, 8), np.int32))
        if want_cams:
            out["cams"] = np.empty((B, 2, CAM), np.float32)
        if want_n:
            out["n_components"] = np.empty(B, np.int32)
        if want_source:
            out["source"] = np.empty(B, np.int32)
        if want_dist:
            out["dist"] = np.empty((B, h // 4, w // 4, 2), np.float32)
        if want_labels:
            out["labels"] = np.empty((B, h // 4, w // 4), np.uint16)
        self._chk(self.L.ht_split_hands_model(self.h, depth.ctypes.data_as(u16), _f(cams), _f(poses), w, h, B, int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far), float(max_dist), int(mode),
                                              int(flags), out["frames"].ctypes.data_as(u16), _f(out["cams"]) if want_cams else None, out["info"].ctypes.data_as(i32),
                                              out["n_components"].ctypes.data_as(i32) if want_n else None, out["source"].ctypes.data_as(i32) if want_source else None,
                                              _f(out["dist"]) if want_dist else None, out["labels"].ctypes.data_as(u16) if want_labels else None))
        return out

    def split_hands_model_dev(self, d_depth, d_cams, d_poses, w, h, B, range_lo, range_hi, max_step, min_pixels, far, max_dist, mode, flags, d_depth_out, d_cams_out, d_info, d_n_components=None, d_source=None,
                              d_dist=None, d_labels=None, stream=None):
        self._chk(self.L.ht_split_hands_model_dev(self.h, d_depth, d_cams, d_poses, int(w), int(h), int(B), int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far), float(max_dist), int(mode), int(flags),
                                                  d_depth_out, d_cams_out, d_info, d_n_components, d_source, d_dist, d_labels, stream))

    def update_two_hands_model(self, depth, cams, range_lo, range_hi, far, max_dist=float("inf"), mode=SPLIT_MODEL_MERGED, side=64, segment_scale=0.17, max_step=65535, min_pixels=1, flags=0, want_cnn=False):
        """update_two_hands_sync with the model split in front, priors the slots' carried state: poses [B,2,nb,7], info i32[B,2,8], source i32[B], and cnn_out [2B,2304] on request
        (ht_update_two_hands_model_sync)"""
        B, h, w, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn, per_frame=2, cam_rows=None)
        info = np.empty((B, 2, 8), np.int32); source = np.empty(B, np.int32)
        i32 = C.POINTER(C.c_int32)
        self._chk(self.L.ht_update_two_hands_model_sync(self.h, int(side), dp, cp, w, h, float(segment_scale), int(range_lo), int(range_hi), int(max_step),
                                                        int(min_pixels), int(far), float(max_dist), int(mode), int(flags), B, pp, info.ctypes.data_as(i32), source.ctypes.data_as(i32), np_))
        return (poses, info, source, cnn) if want_cnn else (poses, info, source)

    def update_two_hands_model_dev(self, side, d_depth, d_cams, w, h, segment_scale, range_lo, range_hi, max_step, min_pixels, far, max_dist, mode, flags, d_start, B, d_poses_out, d_info=None, d_source=None, stream=None):
        self._chk(self.L.ht_update_two_hands_model_dev(self.h, int(side), d_depth, d_cams, int(w), int(h), float(segment_scale), int(range_lo), int(range_hi), int(max_step), int(min_pixels), int(far),
                                                       float(max_dist), int(mode), int(flags), d_start, int(B), d_poses_out, d_info, d_source, stream))

    def update_direct_sync(self, depth, cams, side=128, want_cnn=False):
        """BASELINE configs[4] end to end: depth u16[B,side,side] frames that are their own segment, the net of that input size (ht_update_direct_sync)."""
        B, _, _, dp, cp, poses, cnn, pp, np_ = self._update_io(depth, cams, want_cnn, pixels=side * side)
        self._chk(self.L.ht_update_direct_sync(self.h, dp, cp, int(side), B, pp, np_))
        return (poses, cnn) if want_cnn else (poses, None)

    def update_direct_dev(self, d_depth, d_cams, side, d_start, B, d_poses_out, stream):
        self._chk(self.L.ht_update_direct_dev(self.h, d_depth, d_cams, int(side), d_start, B, d_poses_out, stream))

    def update_cnn_model_sync(self, depth, cams, kickstart=False, segment_scale=0.17):
        """HandTracker::update_cnn_model (handtrack.h:734-741) / kickstart (:743-746): depth u16[B,h,w] -> (othermodel poses [B,nb,7], accepted [B])."""
        depth = _c(depth, np.uint16)
        if depth.ndim == 2:
            depth = depth.reshape(-1, 64, 64)
        B, h, w, dp, cp, poses, _, pp, _ = self._update_io(depth, cams, False)
        acc = np.empty(B, np.int32)
        self._chk(self.L.ht_update_cnn_model_sync(self.h, dp, cp, w, h, float(segment_scale), B, int(bool(kickstart)), pp, _i(acc), None))
        return poses, acc

    def cnn_results(self, n, first=0):
        """(cnn_input [n,4096], cnn_output [n,2304], analysis [n,84]) of the latest update of those slots (HandTracker::cnn_input / cnn_output / cnn_output_analysis)"""
        a = np.empty((n, CNN_IN), np.float32); b = np.empty((n, CNN_OUT), np.float32); c = np.empty((n, ANALYSIS), np.float32)
        self._chk(self.L.ht_get_cnn_results(self.h, first, n, _f(a), _f(b), _f(c)))
        return a, b, c

    def capacity_events(self):
        """(expanding-polytope runs cut short, contacts dropped, solves with angular rows over capacity) since the context was created"""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        self._chk(self.L.ht_capacity_events(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def cnn_layers(self, n, first=0, side=64):
        """(act1 [n,3600], act2 [n,2304], act3 [n,2048], logits [n,2304]) of the latest CNN evaluation (ht_get_cnn_layers); side = 128: the 128x128-input net's
        act1 [n,15376] and act2 [n,12544] (ht_get_cnn_layers_sized; act3 and logits belong to whichever net ran last)."""
        side = int(side)
        n1, n2 = (3600, 2304) if side == 64 else (16 * 31 * 31, 12544)      # any other side: the library refuses it
        a1 = np.zeros((n, n1), np.float32); a2 = np.zeros((n, n2), np.float32); a3 = np.zeros((n, 2048), np.float32); lg = np.zeros((n, 2304), np.float32)
        if side == 64:
            self._chk(self.L.ht_get_cnn_layers(self.h, int(first), int(n), _f(a1), _f(a2), _f(a3), _f(lg)))
        else:
            self._chk(self.L.ht_get_cnn_layers_sized(self.h, side, int(first), int(n), _f(a1), _f(a2), _f(a3), _f(lg)))
        return a1, a2, a3, lg

    def stage_chamber(self, which, B):
        """cloud_chamber rows [B, 5*nb, 16] and their counts (ht_stage_chamber)."""
        rows = np.zeros((B, 5 * self.nb, 16), np.float32); n = np.zeros(B, np.int32)
        self._chk(self.L.ht_stage_chamber(self.h, int(which), int(B), _f(rows), _i(n)))
        return rows, n

    @staticmethod
    def _ragged(rows, width):
        """list of (n_i, width) arrays -> ([B, cap, width] float32, counts int32, cap)"""
        cap = max(1, max((len(r) for r in rows), default=1))
        buf = np.zeros((len(rows), cap, width), np.float32)
        for i, r in enumerate(rows):
            if len(r):
                buf[i, :len(r)] = np.asarray(r, np.float32).reshape(-1, width)
        return buf, np.array([len(r) for r in rows], np.int32), cap

    def fit_rows(self, which, clouds, linears, angulars, microforce=1.0):
        """PhysModel::FitPointCloud(points, linears, angulars, microforce) (physmodel.h:345-356) on model `which` of slots [0, len(clouds)):
        per slot a point cloud (n,3), the caller's linear rows (n,16) and angular rows (n,8)."""
        B = len(clouds)
        pb, pn, pc = self._ragged(clouds, 3); lb, ln, lc = self._ragged(linears, 16); ab, an, ac = self._ragged(angulars, 8)
        self._chk(self.L.ht_fit_rows(self.h, int(which), B, _f(pb), pc, _i(pn), _f(lb), lc, _i(ln), _f(ab), ac, _i(an), float(microforce)))

    def physics_update(self, which, linears, angulars):
        """PhysicsUpdate(rigidbodies, Linears, Angulars) (physics.h:543-587) on model `which`: per slot the caller's rows (n,16) / (n,8) are all there is."""
        B = len(linears)
        lb, ln, lc = self._ragged(linears, 16); ab, an, ac = self._ragged(angulars, 8)
        self._chk(self.L.ht_physics_update(self.h, int(which), B, _f(lb), lc, _i(ln), _f(ab), ac, _i(an)))

    def set_points(self, clouds):
        """Caller-supplied clouds for the stage calls (ht_set_points): one (n_i, 3) array per slot."""
        cap = max(1, max(len(c) for c in clouds))
        buf = np.zeros((len(clouds), cap, 3), np.float32)
        for i, c in enumerate(clouds):
            buf[i, :len(c)] = np.asarray(c, np.float32).reshape(-1, 3)
        n = np.array([len(c) for c in clouds], np.int32)
        self._chk(self.L.ht_set_points(self.h, len(clouds), _f(buf), cap, _i(n)))

    def point_capacity(self):
        n = C.c_int(0)
        self._chk(self.L.ht_point_capacity(self.h, C.byref(n)))
        return n.value

    def reserve_points(self, points):
        self._chk(self.L.ht_reserve_points(self.h, int(points)))

    def frames_overflow(self):
        n = C.c_int(0)
        self._chk(self.L.ht_frames_overflow(self.h, C.byref(n)))
        return n.value

    # -- stages
    def stage_prepare(self, depth, cams):
        depth = _c(depth, np.uint16).reshape(-1, 4096)
        cams = _c(cams, np.float32).reshape(-1, CAM)
        B = depth.shape[0]
        cnn_in = np.empty((B, CNN_IN), np.float32); pts = np.empty((B, MAXPTS, 4), np.float32); n = np.empty(B, np.int32)
        self._chk(self.L.ht_stage_prepare(self.h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), B, _f(cnn_in), _f(pts), _i(n)))
        return cnn_in, pts, n

    def stage_decode(self, cnn_out, cams):
        cnn_out = _c(cnn_out, np.float32).reshape(-1, CNN_OUT)
        cams = _c(cams, np.float32).reshape(-1, CAM)
        an = np.empty((cnn_out.shape[0], ANALYSIS), np.float32)
        self._chk(self.L.ht_stage_decode(self.h, _f(cnn_out), _f(cams), cnn_out.shape[0], _f(an)))
        return an

    def stage_fit_error(self, which, B):
        e = np.empty(B, np.float32)
        self._chk(self.L.ht_stage_fit_error(self.h, which, B, _f(e)))
        return e

    def stage_cloud_rows(self, which, stride, use_cam_origin, B):
        rows = np.empty((B, MAXPTS, ROW), np.float32); n = np.empty(B, np.int32)
        self._chk(self.L.ht_stage_cloud_rows(self.h, which, stride, int(use_cam_origin), B, _f(rows), _i(n)))
        return rows, n

    def stage_contacts(self, which, B, cap=192):
        c = np.empty((B, cap, CONTACT), np.float32); n = np.empty(B, np.int32)
        self._chk(self.L.ht_stage_contacts(self.h, which, B, cap, _f(c), _i(n)))
        return c, n

    def stage_fit(self, B):
        self._chk(self.L.ht_stage_fit(self.h, B))

    def stage_multistep(self, analysis, B):
        analysis = _c(analysis, np.float32).reshape(B, ANALYSIS)
        self._chk(self.L.ht_stage_multistep(self.h, _f(analysis), B))

    def stage_multistep_range(self, analysis, B, from_step, to_step):
        """steps [from_step, to_step) of MultiStepSim alone, from othermodel's current state"""
        analysis = _c(analysis, np.float32).reshape(B, ANALYSIS)
        self._chk(self.L.ht_stage_multistep_range(self.h, _f(analysis), B, int(from_step), int(to_step)))

    def stage_scratch_unibody(self, analysis, B, n_unibody):
        analysis = _c(analysis, np.float32).reshape(B, ANALYSIS)
        self._chk(self.L.ht_stage_scratch_unibody(self.h, _f(analysis), B, n_unibody))

    def row_counts(self, B):
        """Test aid: the cloud-row counts of slots [0, B) as the latest launch that wrote them left them."""
        n = np.empty(B, np.int32)
        self._chk(self.L.ht_debug_row_counts(self.h, B, _i(n)))
        return n

    def stage_scratch_unibody_listed(self, analysis, B, n_unibody, frames, many_frames=False, nlist=None):
        """Test aid: the same for the listed frames alone, through the flagged-frame list (many_frames False: the few-frames build of k_reset).  nlist: the length handed
        to the library where it is not len(frames)."""
        analysis = _c(analysis, np.float32).reshape(B, ANALYSIS)
        frames = _c(frames, np.int32).reshape(-1)
        self._chk(self.L.ht_stage_scratch_unibody_listed(self.h, _f(analysis), B, n_unibody, _i(frames), len(frames) if nlist is None else int(nlist), int(bool(many_frames))))

    # -- profiling
    def profile_enable(self, level=1):
        """0 off; 1 bracket only the dominant kernel (k_solve) with HIP events; 2 bracket every phase (serialises the side streams)."""
        self._chk(self.L.ht_profile_enable(self.h, int(level)))

    def profile_read(self, reset=True):
        names = C.create_string_buffer(64 * 48); ms = np.zeros(64, np.float32); n = np.zeros(64, np.int32); k = C.c_int()
        self._chk(self.L.ht_profile_read(self.h, int(reset), 64, names, 48, _f(ms), _i(n), C.byref(k)))
        out = {}
        for j in range(k.value):
            out[names.raw[48 * j:48 * (j + 1)].split(b"\0", 1)[0].decode()] = (float(ms[j]), int(n[j]))
        return out

    def debug_solve_stats(self, B, reset=True):
        """Per-frame k_solve statistics [B,16] (only filled when HT_DEBUG_SKIP=2048 is set in the environment)."""
        out = np.zeros((B, 16), np.float32)
        self._chk(self.L.ht_debug_solve_stats(self.h, int(B), _f(out), int(reset)))
        return out

    # ---- multi-GPU result gather (RCCL all-gather on the context's communication stream) ----
    def comm_init(self, world, rank, unique_id):
        """Join the RCCL communicator made from `unique_id` (128 bytes from comm_unique_id() on rank 0)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self.L.ht_comm_init(self.h, int(world), int(rank), C.cast(buf, C.c_void_p)))

    def comm_info(self):
        w, r = C.c_int(0), C.c_int(0)
        self._chk(self.L.ht_comm_info(self.h, C.byref(w), C.byref(r)))
        return w.value, r.value

    def gather_poses_dev(self, d_local, d_all, frames, slot, stream=None):
        self._chk(self.L.ht_gather_poses_dev(self.h, C.c_void_p(d_local), C.c_void_p(d_all), int(frames), int(slot), C.c_void_p(stream or 0)))

    def gather_wait(self, slot, stream=None):
        self._chk(self.L.ht_gather_wait(self.h, int(slot), C.c_void_p(stream or 0)))

    def debug_reset_organisation(self):
        """0 / 1: the latest update launched the full-reset branch in its few-frames / many-frames organisation; -1 before the first update"""
        m = C.c_int(-1)
        self._chk(self.L.ht_debug_reset_organisation(self.h, C.byref(m)))
        return m.value

    def gather_wait_host(self, slot):
        self._chk(self.L.ht_gather_wait_host(self.h, int(slot)))

    def debug_reset_flags(self, n):
        """which tracker slots took the full-reset branch (handtrack.h:706-711) in the latest update"""
        f = np.zeros(n, np.int32)
        self._chk(self.L.ht_debug_reset_flags(self.h, f.ctypes.data_as(C.POINTER(C.c_int)), n))
        return f

    def debug_solver_build(self, which):
        """Test aid: pin k_solve's build (0 auto, 1 small, 2 only, 3 mid, 4 tiny = every row array in HBM: placement only, results identical; 5 = the exact-order
        instantiation: the reference's own sweeps, tests/test_gpu_exact_solver.py)."""
        self._chk(self.L.ht_debug_solver_build(self.h, int(which)))

    def debug_contact_kernel(self, which):
        """Test aid: pin the contact kernel's organisation (0 auto, 1 cooperative, 2 lane-per-pair).  Same contacts either way."""
        self._chk(self.L.ht_debug_contact_kernel(self.h, int(which)))

    def debug_stream_edges(self, mode):
        """Test aid: how the edges between an update's streams are made (0 the product's choice, 1 a record and a wait per edge on the events of round 29 and before).
        Waits for the context's work.  Same results either way."""
        self._chk(self.L.ht_debug_stream_edges(self.h, int(mode)))

    def debug_contact_plan(self, B):
        """Test aid: (frames per block of the cooperative kernel, waves per frame of the lane-per-pair kernel) of a contact launch on B frames under the current pin; the
        kernel that does not run has 0."""
        a, b = C.c_int(0), C.c_int(0)
        self._chk(self.L.ht_debug_contact_plan(self.h, int(B), C.byref(a), C.byref(b)))
        return a.value, b.value

    def debug_contact_order(self, work, nfr, epb):
        """Test aid: k_contact_order's table for one launch slot from the per-frame costs `work` (candidates + 2 x patches | polytope runs << 16): [nfr, ceil(B / nfr)],
        table[round, block] = frame, B = no frame; -1 where the launch wrote nothing."""
        work = _c(work, np.int32); B = len(work); blocks = (B + nfr - 1) // nfr
        out = np.empty(blocks * nfr, np.int32)
        self._chk(self.L.ht_debug_contact_order(self.h, _i(work), B, int(nfr), int(epb), _i(out)))
        return out.reshape(nfr, blocks)

    def debug_rank_desc(self, work):
        """Test aid: k_rank_desc's table for one launch slot: the frames of every 4096-frame segment by `work`, largest first, ties by index; -1 where the launch wrote nothing."""
        work = _c(work, np.int32); out = np.empty(len(work), np.int32)
        self._chk(self.L.ht_debug_rank_desc(self.h, _i(work), len(work), _i(out)))
        return out

    def contact_capacity(self):
        """(samples_bound, patches_bound, pool, patch_slots): the most touching samples / five-sample patches a frame of this model can produce, and what the contact kernel holds"""
        v = [C.c_int() for _ in range(4)]
        self._chk(self.L.ht_contact_capacity(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def debug_solve_tables(self, on):
        """Test aid: 0 = k_solve makes every solve's tables in its own prologue (as until round 5), 1 = k_solve_prep makes them beside the contact kernel.  Same results."""
        self._chk(self.L.ht_debug_solve_tables(self.h, int(on)))

    def debug_solve_tables_header(self, B):
        """Tuning aid: the header words [B,32] of the frames' solve tables as the latest k_solve_prep left them."""
        h = np.zeros((B, 32), np.int32)
        self._chk(self.L.ht_debug_solve_tables_header(self.h, B, _i(h)))
        return h

    def debug_contact_stats(self, B, reset=True):
        """Per-frame k_contacts statistics [B,12] + the polytope runs of the frame's wave [B,5] (only filled when HT_DEBUG_SKIP=2048 is set in the environment)."""
        out = np.zeros((B, 24), np.float32)
        self._chk(self.L.ht_debug_contact_stats(self.h, int(B), _f(out), int(reset)))
        return np.concatenate([out[:, 12:], out[:, :5]], axis=1)

    def segment_vr(self, depth, cams, entry_options=0xF, wrange=(0.1, 0.65), diam=0.17):
        """HandSegmentVR (handtrack.h:280-344) for a batch: depth u16[B,h,w], cams [B,12] -> (tiles u16[B,64,64], cams [B,12])."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, CAM)
        tiles = np.empty((B, 64, 64), np.uint16); co = np.empty((B, CAM), np.float32)
        self._chk(self.L.ht_segment_vr(self.h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), w, h, B, int(entry_options), float(wrange[0]), float(wrange[1]), float(diam),
                                       tiles.ctypes.data_as(C.POINTER(C.c_uint16)), _f(co)))
        return tiles, co

    def segment_vr_sized(self, depth, cams, side=128, entry_options=0xF, wrange=(0.1, 0.65), diam=0.17):
        """HandSegmentVR with the tile side a parameter, frames up to 640x480 (ht_segment_vr_sized): depth u16[B,h,w], cams [B,12] -> (tiles u16[B,side,side], cams [B,12])."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, CAM)
        if side not in (64, 128):      # the output cannot be shaped for any other side: the library's own refusal, with nothing to write into
            self._chk(self.L.ht_segment_vr_sized(self.h, int(side), depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), w, h, B, int(entry_options), float(wrange[0]), float(wrange[1]), float(diam), None, None))
        tiles = np.empty((B, side, side), np.uint16); co = np.empty((B, CAM), np.float32)
        self._chk(self.L.ht_segment_vr_sized(self.h, int(side), depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), w, h, B, int(entry_options), float(wrange[0]), float(wrange[1]), float(diam),
                                             tiles.ctypes.data_as(C.POINTER(C.c_uint16)), _f(co)))
        return tiles, co

    def segment_vr_sized_dev(self, side, d_depth, d_cams, w, h, B, d_tiles, d_cams_out, stream=None, entry_options=0xF, wrange=(0.1, 0.65), diam=0.17):
        self._chk(self.L.ht_segment_vr_sized_dev(self.h, int(side), d_depth, d_cams, int(w), int(h), int(B), int(entry_options), float(wrange[0]), float(wrange[1]), float(diam), d_tiles, d_cams_out, stream))

    def _render(self, entry, poses, cams, w, h, far, extra, want_body):
        """a renderer's synchronous entry: `extra` are its arguments between far and B"""
        poses = _c(poses, np.float32).reshape(-1, self.nb, POSE); B = poses.shape[0]
        cams = _c(cams, np.float32).reshape(B, CAM)
        depth = np.empty((B, int(h), int(w)), np.uint16)
        body = np.empty((B, int(h), int(w)), np.int8) if want_body else None
        self._chk(entry(self.h, _f(poses), _f(cams), int(w), int(h), float(far), *extra, B, depth.ctypes.data_as(C.POINTER(C.c_uint16)),
                        body.ctypes.data_as(C.POINTER(C.c_int8)) if want_body else None))
        return (depth, body) if want_body else depth

    def render_depth(self, poses, cams, w, h, far=4.0, want_body=False):
        """FakeDepth (synthetic-tracker.cpp:69-76) for a batch: the context's hand at centre-of-mass poses [B,nb,7], cameras [B,12] ->
        depth u16[B,h,w] (and the hit body int8[B,h,w], -1 = background, with want_body)."""
        return self._render(self.L.ht_render_depth, poses, cams, w, h, far, (), want_body)

    def render_depth_dev(self, d_poses, d_cams, w, h, far, B, d_depth, d_body=None, stream=None):
        """ht_render_depth_dev: device pointers (poses [B,nb,7], cams [B,12] -> depth u16[B,h,w], body int8[B,h,w] or None), asynchronous on `stream`."""
        self._chk(self.L.ht_render_depth_dev(self.h, d_poses, d_cams, int(w), int(h), float(far), int(B), d_depth, d_body, stream))

    def render_mesh_depth(self, poses, cams, w, h, far=4.0, pixel_offset=0.0, want_body=False):
        """The hand's subdivision surface (GetMeshes(true)) ray-cast for a batch, bit-identical to HostModel.render_mesh: poses [B,nb,7], cameras [B,12] ->
        depth u16[B,h,w] (and the hit body int8[B,h,w], -1 = background, with want_body).  pixel_offset 0 / far 4 matches render_depth's frames,
        0.5 / 0.85 the application's GL frames."""
        return self._render(self.L.ht_render_mesh_depth, poses, cams, w, h, far, (float(pixel_offset),), want_body)

    def render_mesh_depth_dev(self, d_poses, d_cams, w, h, far, pixel_offset, B, d_depth, d_body=None, stream=None):
        """ht_render_mesh_depth_dev: device pointers, asynchronous on `stream`."""
        self._chk(self.L.ht_render_mesh_depth_dev(self.h, d_poses, d_cams, int(w), int(h), float(far), float(pixel_offset), int(B), d_depth, d_body, stream))

    def raster_mesh_depth(self, poses, cams, w, h, far=4.0, pixel_offset=0.0, want_body=False):
        """The same surface through the z-buffer rasteriser (ht_raster_mesh_depth), bit-identical to HostModel.raster_mesh: shapes and conventions as
        render_mesh_depth.  Its definition is its own (ht_mi355x.h), within one count of the ray cast where both pick the same triangle."""
        return self._render(self.L.ht_raster_mesh_depth, poses, cams, w, h, far, (float(pixel_offset),), want_body)

    def raster_mesh_depth_dev(self, d_poses, d_cams, w, h, far, pixel_offset, B, d_depth, d_body=None, stream=None):
        """ht_raster_mesh_depth_dev: device pointers, asynchronous on `stream`."""
        self._chk(self.L.ht_raster_mesh_depth_dev(self.h, d_poses, d_cams, int(w), int(h), float(far), float(pixel_offset), int(B), d_depth, d_body, stream))

    def raster_scene_depth(self, poses, cams, w, h, hands=None, far=4.0, pixel_offset=0.0, bg=None, want_hand=True, want_body=True, want_visible=True, in_place=False):
        """Scenes of H hands a frame, each right or left, in one z-buffer pass (ht_raster_scene_depth), bit-identical to HostModel.raster_scene: poses [B,H,nb,7],
        cameras [B,12], hands u8[B,H] (SCENE_RIGHT, SCENE_ABSENT, anything else left; None: all right), bg u16[B,h,w] or None -> a dict of depth u16[B,h,w] and, as asked
        for, hand int8[B,h,w], body int8[B,h,w], visible int32[B,H].  in_place: bg itself is the depth buffer (bg == depth) and is returned composed."""
        poses = _c(poses, np.float32); B, H = poses.shape[0], poses.shape[1]
        poses = poses.reshape(B, H, self.nb, POSE); cams = _c(cams, np.float32).reshape(B, CAM)
        hands = None if hands is None else _c(hands, np.uint8).reshape(B, H)
        bg = None if bg is None else _c(bg, np.uint16).reshape(B, int(h), int(w))
        depth = bg if (in_place and bg is not None) else np.empty((B, int(h), int(w)), np.uint16)
        hand = np.empty((B, int(h), int(w)), np.int8) if want_hand else None
        body = np.empty((B, int(h), int(w)), np.int8) if want_body else None
        visible = np.empty((B, H), np.int32) if want_visible else None
        u16p, i8p = C.POINTER(C.c_uint16), C.POINTER(C.c_int8)
        self._chk(self.L.ht_raster_scene_depth(self.h, _f(poses), hands.ctypes.data_as(C.POINTER(C.c_uint8)) if hands is not None else None, H, _f(cams), int(w), int(h), float(far), float(pixel_offset), B,
                                               bg.ctypes.data_as(u16p) if bg is not None else None, depth.ctypes.data_as(u16p), hand.ctypes.data_as(i8p) if want_hand else None,
                                               body.ctypes.data_as(i8p) if want_body else None, _i(visible) if want_visible else None))
        out = dict(depth=depth)
        if want_hand: out["hand"] = hand
        if want_body: out["body"] = body
        if want_visible: out["visible"] = visible
        return out

    def raster_scene_depth_dev(self, d_poses, d_hands, H, d_cams, w, h, far, pixel_offset, B, d_bg, d_depth, d_hand=None, d_body=None, d_visible=None, stream=None):
        """ht_raster_scene_depth_dev: device pointers (d_hands, d_bg and the label outputs may be None), asynchronous on `stream`; d_bg == d_depth composes in place."""
        self._chk(self.L.ht_raster_scene_depth_dev(self.h, d_poses, d_hands, int(H), d_cams, int(w), int(h), float(far), float(pixel_offset), int(B), d_bg, d_depth, d_hand, d_body, d_visible, stream))

    # -- joint coordinates (ht_mi355x.h "joint coordinates"): c = (s.x, s.y, t.z) per joint; com_poses: centre-of-mass poses instead of user poses
    def joint_coords(self, poses, com_poses=False, want_gaps=False):
        """poses [B,nb,7] -> coords [B,nj,3] (and the joints' anchor gaps [B,nj] with want_gaps)."""
        poses = _c(poses, np.float32).reshape(-1, self.nb, POSE); B = poses.shape[0]
        coords = np.empty((B, self.nj, 3), np.float32); gaps = np.empty((B, self.nj), np.float32) if want_gaps else None
        self._chk(self.L.ht_joint_coords(self.h, _f(poses), B, JOINTS_COM_POSES if com_poses else 0, _f(coords), _f(gaps) if want_gaps else None))
        return (coords, gaps) if want_gaps else coords

    def joint_coords_dev(self, d_poses, B, d_coords, d_gaps=None, com_poses=False, stream=None):
        self._chk(self.L.ht_joint_coords_dev(self.h, d_poses, int(B), JOINTS_COM_POSES if com_poses else 0, d_coords, d_gaps, stream))

    def joint_pose(self, roots, coords, com_poses=False):
        """Forward kinematics: body 0's poses [B,7] and coords [B,nj,3] -> poses [B,nb,7].  Coordinates outside a unit quaternion's are refused."""
        roots = _c(roots, np.float32).reshape(-1, POSE); B = roots.shape[0]
        coords = _c(coords, np.float32).reshape(B, self.nj, 3)
        poses = np.empty((B, self.nb, POSE), np.float32)
        self._chk(self.L.ht_joint_pose(self.h, _f(roots), _f(coords), B, JOINTS_COM_POSES if com_poses else 0, _f(poses)))
        return poses

    def joint_pose_dev(self, d_roots, d_coords, B, d_poses, com_poses=False, stream=None):
        """ht_joint_pose_dev: device pointers, asynchronous on `stream`; out-of-range coordinates are clamped, not refused."""
        self._chk(self.L.ht_joint_pose_dev(self.h, d_roots, d_coords, int(B), JOINTS_COM_POSES if com_poses else 0, d_poses, stream))

    def sample_poses(self, roots, seed, first_index=0, spread=1.0, com_poses=False, want_coords=False, enhanced=False):
        """B poses inside the joint limits, sample i drawn from (seed, first_index + i): roots [B,7] -> poses [B,nb,7] (and coords [B,nj,3]);
        enhanced: HandModelEnhancements' couplings (fingertip joints follow their knuckles, no abduction on a clenched finger)."""
        roots = _c(roots, np.float32).reshape(-1, POSE); B = roots.shape[0]
        poses = np.empty((B, self.nb, POSE), np.float32); coords = np.empty((B, self.nj, 3), np.float32) if want_coords else None
        self._chk(self.L.ht_sample_poses(self.h, _f(roots), B, int(seed), int(first_index), float(spread), (JOINTS_COM_POSES if com_poses else 0) | (SAMPLE_ENHANCED if enhanced else 0), _f(poses), _f(coords) if want_coords else None))
        return (poses, coords) if want_coords else poses

    def sample_poses_dev(self, d_roots, B, seed, first_index, spread, d_poses, d_coords=None, com_poses=False, enhanced=False, stream=None):
        self._chk(self.L.ht_sample_poses_dev(self.h, d_roots, int(B), int(seed), int(first_index), float(spread), (JOINTS_COM_POSES if com_poses else 0) | (SAMPLE_ENHANCED if enhanced else 0), d_poses, d_coords, stream))

    # -- tracking accuracy (ht_mi355x.h "tracking accuracy"): keypoints, keypoint errors, depth residuals
    def keypoint_table(self, which):
        """A built-in keypoint table (KP_FEATURE8, KP_SKELETON) of the model as ht_scale left it -> (bones i32[K], offsets f32[K,3], rel i32[K])."""
        K = C.c_int()
        self._chk(self.L.ht_keypoint_table(self.h, int(which), C.byref(K), None, None, None))
        bones, off, rel = np.empty(K.value, np.int32), np.empty((K.value, 3), np.float32), np.empty(K.value, np.int32)
        self._chk(self.L.ht_keypoint_table(self.h, int(which), None, _i(bones), _f(off), _i(rel)))
        return bones, off, rel

    @staticmethod
    def _kp_table(table):
        """table: KP_FEATURE8 / KP_SKELETON, or a caller table (bones [K], offsets [K,3], rel [K]) -> (which, K, keep-alive arrays, the three pointers)"""
        if isinstance(table, (int, np.integer)):
            return int(table), 0, (), (None, None, None)
        bones, off, rel = _c(table[0], np.int32).reshape(-1), _c(table[1], np.float32).reshape(-1, 3), _c(table[2], np.int32).reshape(-1)
        if not (len(off) == len(bones) == len(rel)):
            raise ValueError("a keypoint table is (bones [K], offsets [K,3], rel [K])")
        return KP_CALLER, len(bones), (bones, off, rel), (_i(bones), _f(off), _i(rel))

    def keypoints(self, poses, table=KP_FEATURE8, com_poses=False, hands=None, cams=None, depth=None, near_tol=0.03, far_tol=0.02, want_xyz=True, want_zc=True):
        """poses [B,nb,7] (user poses; com_poses: centre-of-mass poses) -> dict(xyz f32[B,K,3]; with cams [B,12]: pix f32[B,K,2], zc f32[B,K]; with depth
        u16[B,h,w] as well: vis u8[B,K], 0 visible, 1 occluded, 2 nothing there, 3 outside the image, 4 behind the camera).  hands u8[B]: left hands."""
        poses = _c(poses, np.float32).reshape(-1, self.nb, POSE); B = poses.shape[0]
        which, K, keep, tp = self._kp_table(table)
        if which != KP_CALLER:
            Kc = C.c_int(); self._chk(self.L.ht_keypoint_table(self.h, which, C.byref(Kc), None, None, None)); K = Kc.value
        u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
        hands = None if hands is None else _c(hands, np.uint8).reshape(B)
        cams = None if cams is None else _c(cams, np.float32).reshape(B, CAM)
        h = w = 0
        if depth is not None:
            depth = _c(depth, np.uint16); h, w = depth.shape[-2:]; depth = depth.reshape(B, h, w)
        out = {}
        if want_xyz:
            out["xyz"] = np.empty((B, K, 3), np.float32)
        if cams is not None:
            out["pix"] = np.empty((B, K, 2), np.float32)
            if want_zc:
                out["zc"] = np.empty((B, K), np.float32)
            if depth is not None:
                out["vis"] = np.empty((B, K), np.uint8)
        g = lambda n: _f(out[n]) if n in out else None
        self._chk(self.L.ht_keypoints(self.h, _f(poses), B, KP_COM_POSES if com_poses else 0, which, K, tp[0], tp[1], tp[2], None if hands is None else hands.ctypes.data_as(u8p),
                                      None if cams is None else _f(cams), None if depth is None else depth.ctypes.data_as(u16p), int(w), int(h), float(near_tol), float(far_tol),
                                      g("xyz"), g("pix"), g("zc"), out["vis"].ctypes.data_as(u8p) if "vis" in out else None))
        return out

    def keypoints_dev(self, d_poses, B, table, d_xyz, d_pix=None, d_zc=None, d_vis=None, com_poses=False, d_hands=None, d_cams=None, d_depth=None, w=0, h=0, near_tol=0.03, far_tol=0.02, stream=None):
        """ht_keypoints_dev: device pointers (the table stays a host table), asynchronous on `stream`."""
        which, K, keep, tp = self._kp_table(table)
        self._chk(self.L.ht_keypoints_dev(self.h, d_poses, int(B), KP_COM_POSES if com_poses else 0, which, K, tp[0], tp[1], tp[2], d_hands, d_cams, d_depth, int(w), int(h), float(near_tol), float(far_tol),
                                          d_xyz, d_pix, d_zc, d_vis, stream))

    # -- keypoint fit (ht_mi355x.h "keypoint fit"): from keypoint targets to a pose
    def _kp_count(self, which, K):
        if which != KP_CALLER:
            Kc = C.c_int(); self._chk(self.L.ht_keypoint_table(self.h, which, C.byref(Kc), None, None, None)); K = Kc.value
        return K

    def fit_keypoints(self, B, table=KP_SKELETON, xyz=None, pix=None, cams=None, weights=None, kind=None, options=None, which_model=0, want_poses=True, want_resid=True):
        """Fits model which_model of slots [0,B) from its current state to the targets: xyz f32[B,K,3] for the keypoints of kind 0, pix f32[B,K,2] in cams f32[B,12]
        for those of kind 1 (kind i32[K], None: all 0), weights f32[B,K] in [0,1] (0 or a NaN target: not annotated).  options: a KpFit (None: kpfit_default()).
        -> dict(poses f32[B,nb,7] user poses, resid f32[B,2,K] before and after; -1: absent)."""
        which, K, keep, tp = self._kp_table(table)
        K = self._kp_count(which, K); B = int(B)
        a = lambda x, tail: None if x is None else _c(x, np.float32).reshape((B, K) + tail)
        xyz, pix, weights = a(xyz, (3,)), a(pix, (2,)), a(weights, ())
        cams = None if cams is None else _c(cams, np.float32).reshape(B, CAM)
        kind = None if kind is None else _c(kind, np.int32).reshape(K)
        out = {}
        if want_poses:
            out["poses"] = np.empty((B, self.nb, POSE), np.float32)
        if want_resid:
            out["resid"] = np.empty((B, 2, K), np.float32)
        g = lambda x: None if x is None else _f(x)
        self._chk(self.L.ht_fit_keypoints(self.h, int(which_model), B, which, K if which == KP_CALLER else 0, tp[0], tp[1], tp[2], None if kind is None else _i(kind), g(xyz), g(pix), g(weights), g(cams),
                                          None if options is None else C.byref(options), g(out.get("poses")), g(out.get("resid"))))
        return out

    def fit_keypoints_dev(self, B, table, d_xyz=None, d_pix=None, d_cams=None, d_weights=None, kind=None, options=None, which_model=0, d_poses=None, d_resid=None, stream=None):
        """ht_fit_keypoints_dev: device pointers (the table and kind stay host arrays), only enqueued on `stream`."""
        which, K, keep, tp = self._kp_table(table)
        kind = None if kind is None else _c(kind, np.int32).reshape(-1)
        self._chk(self.L.ht_fit_keypoints_dev(self.h, int(which_model), int(B), which, K, tp[0], tp[1], tp[2], None if kind is None else _i(kind), d_xyz, d_pix, d_weights, d_cams,
                                              None if options is None else C.byref(options), d_poses, d_resid, stream))

    # -- several views (ht_mi355x.h "several views"): one hand from V <= VIEWS_MAX depth cameras and their mirrors
    def views_default(self, **kw):
        """ht_views_default (range {0.1, drangey}, fraction = subsample_fraction, mirror_eps 0.02), then the fields given"""
        o = Views()
        self._chk(self.L.ht_views_default(self.h, C.byref(o)))
        for k, v in kw.items():
            if k not in dict(Views._fields_):
                raise TypeError("ht_views has no field %r" % k)
            setattr(o, k, v)
        return o

    @staticmethod
    def _views_io(depth, cams, planes):
        depth = _c(depth, np.uint16)
        B, V, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, V, CAM)
        planes = None if planes is None else _c(planes, np.float32).reshape(B, V, 4)
        return depth, cams, planes, B, V, h, w

    def fuse_views(self, depth, cams, planes=None, options=None, cap=None):
        """depth u16[B,V,h,w], cams f32[B,V,12] posed in one tracking space, planes f32[B,V,4] or None -> dict(points f32[B,cap,4] (x y z source; cap None: the most the
        views can carry), npoints i32[B], per_source i32[B,2V], origins f32[B,2V,3], cut).  The cloud stays in slots [0,B) for fit_views / stage_view_rows."""
        depth, cams, planes, B, V, h, w = self._views_io(depth, cams, planes)
        if cap is None:
            fr = (options.fraction if options is not None else self.views_default().fraction) or 1
            cap = max(V * ((w * h + fr - 1) // max(fr, 1)), 1)
        out = dict(points=np.zeros((B, cap, 4), np.float32), npoints=np.zeros(B, np.int32), per_source=np.zeros((B, 2 * V), np.int32), origins=np.zeros((B, 2 * V, 3), np.float32))
        cut = C.c_int(0)
        self._chk(self.L.ht_fuse_views(self.h, depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), None if planes is None else _f(planes), w, h, V, B, None if options is None else C.byref(options),
                                       _f(out["points"]), int(cap), _i(out["npoints"]), _i(out["per_source"]), _f(out["origins"]), C.byref(cut)))
        out["cut"] = cut.value
        return out

    def fuse_views_dev(self, d_depth, d_cams, w, h, V, B, d_planes=None, options=None, d_npoints=None, d_per_source=None, d_origins=None, d_cut=None, stream=None):
        """ht_fuse_views_dev: device pointers, only enqueued on `stream`; the cloud is left in slots [0,B)."""
        self._chk(self.L.ht_fuse_views_dev(self.h, d_depth, d_cams, d_planes, int(w), int(h), int(V), int(B), None if options is None else C.byref(options), d_npoints, d_per_source, d_origins, d_cut, stream))

    def stage_view_rows(self, which, B, cap=None):
        """The cloud rows of the fused points of slots [0,B), each from its own ray origin -> (rows f32[B,cap,16], nrows i32[B]); cap None: the context's point capacity."""
        if cap is None:
            cap = self.point_capacity()
        rows = np.zeros((B, cap, ROW), np.float32); n = np.zeros(B, np.int32)
        self._chk(self.L.ht_stage_view_rows(self.h, int(which), int(B), _f(rows), int(cap), _i(n)))
        return rows, n

    def fit_views(self, which, B, passes=1, want_poses=True):
        """`passes` fits of model `which` of slots [0,B) against the fused cloud -> the user poses f32[B,nb,7] (or None)."""
        poses = np.empty((B, self.nb, POSE), np.float32) if want_poses else None
        self._chk(self.L.ht_fit_views(self.h, int(which), int(B), int(passes), None if poses is None else _f(poses)))
        return poses

    def fit_views_dev(self, which, B, passes=1, d_poses=None, stream=None):
        self._chk(self.L.ht_fit_views_dev(self.h, int(which), int(B), int(passes), d_poses, stream))

    def update_views_sync(self, depth, cams, planes=None, side=64, segment_scale=0.17, options=None, passes=3, want_cnn=False):
        """ht_update_frames_sized_sync on view 0, then the fused cloud of all views and `passes` fits: depth u16[B,V,h,w], cams f32[B,V,12] (view 0's pose identity)."""
        depth, cams, planes, B, V, h, w = self._views_io(depth, cams, planes)
        poses = np.empty((B, self.nb, POSE), np.float32); cnn = np.empty((B, CNN_OUT), np.float32) if want_cnn else None
        self._chk(self.L.ht_update_views_sync(self.h, int(side), depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), None if planes is None else _f(planes), w, h, V, float(segment_scale), B,
                                              None if options is None else C.byref(options), int(passes), _f(poses), None if cnn is None else _f(cnn)))
        return (poses, cnn) if want_cnn else poses

    def update_views_dev(self, side, d_depth, d_cams, w, h, V, segment_scale, d_start, B, d_poses_out, d_planes=None, options=None, passes=3, stream=None):
        self._chk(self.L.ht_update_views_dev(self.h, int(side), d_depth, d_cams, d_planes, int(w), int(h), int(V), float(segment_scale), d_start, int(B), None if options is None else C.byref(options),
                                             int(passes), d_poses_out, stream))

    # -- a view's extrinsics from the tracked hand (ht_mi355x.h "a view's extrinsics")
    def calib_default(self, **kw):
        """ht_calib_default (range {0.1, drangey}, fraction = subsample_fraction, RIG, 10 iterations, max_dist 0.03, damping 1e-3, min_points 12, centre 0), then the fields given"""
        o = Calib()
        self._chk(self.L.ht_calib_default(self.h, C.byref(o)))
        for k, v in kw.items():
            if k not in dict(Calib._fields_):
                raise TypeError("ht_calib has no field %r" % k)
            setattr(o, k, tuple(float(x) for x in v) if k == "centre" else v)
        return o

    def calibrate_view(self, depth, cams, poses=None, which=0, options=None):
        """depth u16[B,h,w] and cams f32[B,12] of ONE view (its guess in cams[:,5:12]), poses f32[B,nb,7] centre-of-mass poses in tracking space or None for the state of
        model `which` of slots [0,B) -> (T f32[N,7] mapping the view's camera space to tracking space, stats f64[iterations + 1,N,27]); N = 1 (RIG) or B (PER_SLOT)."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, CAM)
        poses = None if poses is None else _c(poses, np.float32).reshape(B, self.nb, POSE)
        o = options if options is not None else self.calib_default()
        N = B if o.mode == CALIB_PER_SLOT else 1
        T = np.zeros((N, 7), np.float32); stats = np.zeros((max(o.iterations, 0) + 1, N, CALIB_STATS), np.float64)
        self._chk(self.L.ht_calibrate_view(self.h, int(which), None if poses is None else _f(poses), depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), w, h, B, C.byref(o), _f(T),
                                           stats.ctypes.data_as(C.POINTER(C.c_double))))
        return T, stats

    def calibrate_view_dev(self, d_depth, d_cams, w, h, B, d_T_out, d_stats, d_poses=None, which=0, options=None, stream=None):
        """ht_calibrate_view_dev: device pointers, only enqueued on `stream`."""
        self._chk(self.L.ht_calibrate_view_dev(self.h, int(which), d_poses, d_depth, d_cams, int(w), int(h), int(B), None if options is None else C.byref(options), d_T_out, d_stats, stream))

    # -- the hand's size from tracked frames (ht_mi355x.h "the hand's size")
    def size_default(self, **kw):
        """ht_size_default (ht_calib_default's range, fraction, max_dist, damping and min_points; SHARED, free_pose 1, 10 iterations, scale0 1 in [0.5, 2]), then the fields given"""
        o = Size()
        self._chk(self.L.ht_size_default(self.h, C.byref(o)))
        for k, v in kw.items():
            if k not in dict(Size._fields_):
                raise TypeError("ht_size has no field %r" % k)
            setattr(o, k, v)
        return o

    def estimate_scale(self, depth, cams, poses=None, which=0, options=None):
        """depth u16[B,h,w] and cams f32[B,12] of ONE view, poses f32[B,nb,7] centre-of-mass poses in tracking space or None for the state of model `which` of slots [0,B)
        -> (scale f32[N], T f32[B,7], stats f64[iterations + 1, size_row(N, B)]); N = 1 (SHARED) or B (PER_SLOT).  Applying the scale is ht_scale's."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, CAM)
        poses = None if poses is None else _c(poses, np.float32).reshape(B, self.nb, POSE)
        o = options if options is not None else self.size_default()
        N = B if o.mode == SIZE_PER_SLOT else 1
        scale = np.zeros(N, np.float32); T = np.zeros((B, 7), np.float32); stats = np.zeros((max(o.iterations, 0) + 1, size_row(N, B)), np.float64)
        self._chk(self.L.ht_estimate_scale(self.h, int(which), None if poses is None else _f(poses), depth.ctypes.data_as(C.POINTER(C.c_uint16)), _f(cams), w, h, B, C.byref(o), _f(scale), _f(T),
                                           stats.ctypes.data_as(C.POINTER(C.c_double))))
        return scale, T, stats

    def estimate_scale_dev(self, d_depth, d_cams, w, h, B, d_scale_out, d_T_out, d_stats, d_poses=None, which=0, options=None, stream=None):
        """ht_estimate_scale_dev: device pointers, only enqueued on `stream`."""
        self._chk(self.L.ht_estimate_scale_dev(self.h, int(which), d_poses, d_depth, d_cams, int(w), int(h), int(B), None if options is None else C.byref(options), d_scale_out, d_T_out, d_stats, stream))

    def keypoint_errors(self, a, b, thr=()):
        """a, b f32[B,K,3] -> dict(dist f32[B,K], frame f32[B,2] (mean, max), sum_kp f64[K], hits_kp i64[T], hits_frame i64[T], and from them mean_kp f64[K],
        mean f64, pck f64[T] = hits_kp / (B K), success f64[T] = hits_frame / B)."""
        a = _c(a, np.float32); B, K = a.shape[0], a.shape[1]; a = a.reshape(B, K, 3); b = _c(b, np.float32).reshape(B, K, 3)
        thr = _c(thr, np.float32).reshape(-1); T = len(thr)
        dist, frame = np.empty((B, K), np.float32), np.empty((B, 2), np.float32)
        sum_kp, hk, hf = np.zeros(K, np.float64), np.zeros(T, np.int64), np.zeros(T, np.int64)
        dp, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int64)
        self._chk(self.L.ht_keypoint_errors(self.h, _f(a), _f(b), B, K, _f(thr) if T else None, T, _f(dist), _f(frame), sum_kp.ctypes.data_as(dp), hk.ctypes.data_as(i64p) if T else None,
                                            hf.ctypes.data_as(i64p) if T else None))
        n = max(B, 1)
        return dict(dist=dist, frame=frame, sum_kp=sum_kp, hits_kp=hk, hits_frame=hf, mean_kp=sum_kp / n, mean=sum_kp.sum() / (n * K), pck=hk / float(n * K), success=hf / float(n))

    def keypoint_errors_dev(self, d_a, d_b, B, K, thr, d_dist=None, d_frame=None, d_sum_kp=None, d_hits_kp=None, d_hits_frame=None, stream=None):
        """ht_keypoint_errors_dev: device pointers (thr stays a host array), asynchronous on `stream`."""
        thr = _c(thr, np.float32).reshape(-1)
        self._chk(self.L.ht_keypoint_errors_dev(self.h, d_a, d_b, int(B), int(K), _f(thr) if len(thr) else None, len(thr), d_dist, d_frame, d_sum_kp, d_hits_kp, d_hits_frame, stream))

    @staticmethod
    def depth_figures(info, depth_scale=None):
        """info i64[B,8] -> dict(info, iou f64[B] (NaN for two empty frames), close f64[B] = n_close / n_both, mean_abs, rms, max_abs in raw units, or in metres with
        depth_scale (a scalar or [B])) -- host arithmetic on the exact integers."""
        info = np.asarray(info, np.int64); f = info.astype(np.float64)
        s = 1.0 if depth_scale is None else np.asarray(depth_scale, np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return dict(info=info, iou=f[:, 2] / (f[:, 0] + f[:, 1] - f[:, 2]), close=f[:, 3] / f[:, 2], mean_abs=f[:, 4] / f[:, 2] * s, rms=np.sqrt(f[:, 5] / f[:, 2]) * s, max_abs=f[:, 6] * s)

    def depth_compare(self, a, b, lo, hi, tol=0, depth_scale=None):
        """a, b u16[B,h,w] -> depth_figures of info i64[B,8]: n_a, n_b, n_both, n_close, sum |a-b|, sum (a-b)^2, max |a-b|, 0 over the pixels with lo <= p < hi."""
        a = _c(a, np.uint16); B, h, w = a.shape; b = _c(b, np.uint16).reshape(B, h, w)
        info = np.zeros((B, 8), np.int64); u16p = C.POINTER(C.c_uint16)
        self._chk(self.L.ht_depth_compare(self.h, a.ctypes.data_as(u16p), b.ctypes.data_as(u16p), w, h, B, int(lo), int(hi), int(tol), info.ctypes.data_as(C.POINTER(C.c_int64))))
        return self.depth_figures(info, depth_scale)

    def depth_compare_dev(self, d_a, d_b, w, h, B, lo, hi, tol, d_info, stream=None):
        self._chk(self.L.ht_depth_compare_dev(self.h, d_a, d_b, int(w), int(h), int(B), int(lo), int(hi), int(tol), d_info, stream))

    def pose_depth_residual(self, poses, cams, depth, lo, hi, tol=0, far=4.0, com_poses=False, want_rendered=False):
        """Poses against frames: poses [B,nb,7] rendered as ht_render_depth does in each frame's camera and compared with depth u16[B,h,w] (a = observed, b = rendered)
        -> depth_figures in metres (and rendered u16[B,h,w] with want_rendered).  Choose hi <= far / depth_scale to keep the rendered background out."""
        return self._pose_residual(self.L.ht_pose_depth_residual, poses, cams, depth, lo, hi, tol, far, com_poses, want_rendered)

    def pose_mesh_residual(self, poses, cams, depth, lo, hi, tol=0, far=4.0, com_poses=False, want_rendered=False):
        """pose_depth_residual against the hand's subdivision surface: the renderer is raster_mesh_depth at pixel offset 0 (ht_pose_mesh_residual)."""
        return self._pose_residual(self.L.ht_pose_mesh_residual, poses, cams, depth, lo, hi, tol, far, com_poses, want_rendered)

    def pose_mesh_residual_dev(self, d_poses, d_cams, d_depth, w, h, B, lo, hi, tol, d_info, d_rendered=None, far=4.0, com_poses=False, stream=None):
        self._chk(self.L.ht_pose_mesh_residual_dev(self.h, d_poses, d_cams, d_depth, int(w), int(h), int(B), KP_COM_POSES if com_poses else 0, float(far), int(lo), int(hi), int(tol), d_info, d_rendered, stream))

    def _pose_residual(self, entry, poses, cams, depth, lo, hi, tol, far, com_poses, want_rendered):
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        poses = _c(poses, np.float32).reshape(B, self.nb, POSE); cams = _c(cams, np.float32).reshape(B, CAM)
        info = np.zeros((B, 8), np.int64); rendered = np.empty((B, h, w), np.uint16) if want_rendered else None
        u16p = C.POINTER(C.c_uint16)
        self._chk(entry(self.h, _f(poses), _f(cams), depth.ctypes.data_as(u16p), w, h, B, KP_COM_POSES if com_poses else 0, float(far), int(lo), int(hi), int(tol),
                        info.ctypes.data_as(C.POINTER(C.c_int64)), rendered.ctypes.data_as(u16p) if want_rendered else None))
        out = self.depth_figures(info, cams[:, 4])
        if want_rendered:
            out["rendered"] = rendered
        return out

    def pose_depth_residual_dev(self, d_poses, d_cams, d_depth, w, h, B, lo, hi, tol, d_info, d_rendered=None, far=4.0, com_poses=False, stream=None):
        self._chk(self.L.ht_pose_depth_residual_dev(self.h, d_poses, d_cams, d_depth, int(w), int(h), int(B), KP_COM_POSES if com_poses else 0, float(far), int(lo), int(hi), int(tol), d_info, d_rendered, stream))

    def sensor_filter(self, kind, depth, cams, ir=None, background=None, max_width=320):
        """RSCam::FilterIvy / FilterDS4 (dcam.h:174-226) for a batch of raw frames: depth u16[B,h,w], cams [B,12], ir u8[B,h,w] (DS4), background u16[B,h,w]
        (DS4, optional) -> (depth u16[B,h_out,w_out], cams [B,12])."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        cams = _c(cams, np.float32).reshape(B, CAM)
        ir = None if ir is None else _c(ir, np.uint8); background = None if background is None else _c(background, np.uint16)
        for a in (ir, background):
            if a is not None and a.shape != depth.shape:
                raise ValueError("ir and background have the frames' shape")
        try:
            wo, ho = sensor_out_dims(kind, w, h, max_width)
        except ValueError:
            wo, ho = w, h      # the call below refuses it, with the library's message
        out = np.empty((B, ho, wo), np.uint16); co = np.empty((B, CAM), np.float32)
        u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
        self._chk(self.L.ht_sensor_filter(self.h, int(kind), depth.ctypes.data_as(u16p), None if ir is None else ir.ctypes.data_as(u8p), _f(cams), w, h, B, int(max_width),
                                          None if background is None else background.ctypes.data_as(u16p), out.ctypes.data_as(u16p), _f(co)))
        return out, co

    def sensor_filter_dev(self, kind, d_depth, d_ir, d_cams, w, h, B, max_width, d_background, d_depth_out, d_cams_out, stream=None):
        """ht_sensor_filter_dev: device pointers (d_ir / d_background may be None), asynchronous on `stream`."""
        self._chk(self.L.ht_sensor_filter_dev(self.h, int(kind), d_depth, d_ir, d_cams, int(w), int(h), int(B), int(max_width), d_background, d_depth_out, d_cams_out, stream))

    def sensor_background(self, depth, background=None, fudge=3):
        """RSCam::addbackground (dcam.h:157-162) for a batch: depth u16[B,h,w] folded into the model background u16[B,h,w] (None: a model that starts at 4096);
        returns the new model."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        init = background is None
        bg = np.empty(depth.shape, np.uint16) if init else np.array(background, dtype=np.uint16, order="C")
        if bg.shape != depth.shape:
            raise ValueError("the background model has the frames' shape")
        u16p = C.POINTER(C.c_uint16)
        self._chk(self.L.ht_sensor_background(self.h, depth.ctypes.data_as(u16p), w, h, B, int(fudge), int(init), bg.ctypes.data_as(u16p)))
        return bg

    def sensor_background_dev(self, d_depth, w, h, B, fudge, init, d_background, stream=None):
        """ht_sensor_background_dev: device pointers, asynchronous on `stream`."""
        self._chk(self.L.ht_sensor_background_dev(self.h, d_depth, int(w), int(h), int(B), int(fudge), int(bool(init)), d_background, stream))

    def sensor_simulate(self, kind, depth, noise, want_ir=None):
        """ht_sensor_simulate: clean rendered frames u16[B,h,w] -> raw frames of camera `kind` under the noise set `noise` (SensorNoise; sensor_noise_default);
        frame f is stream noise.first_index + f.  Returns (depth u16[B,h,w], ir u8[B,h,w] or None); want_ir defaults to what the kind needs (DS4)."""
        depth = _c(depth, np.uint16); B, h, w = depth.shape
        if want_ir is None:
            want_ir = int(kind) == SENSOR_DS4
        out = np.empty((B, h, w), np.uint16); ir = np.empty((B, h, w), np.uint8) if want_ir else None
        u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
        self._chk(self.L.ht_sensor_simulate(self.h, int(kind), depth.ctypes.data_as(u16p), w, h, B, C.byref(noise), out.ctypes.data_as(u16p), ir.ctypes.data_as(u8p) if want_ir else None))
        return out, ir

    def sensor_simulate_dev(self, kind, d_depth, w, h, B, noise, d_depth_out, d_ir_out=None, stream=None):
        """ht_sensor_simulate_dev: device pointers (d_ir_out may be None for Ivy), asynchronous on `stream`; `noise` is read now and travels by value."""
        self._chk(self.L.ht_sensor_simulate_dev(self.h, int(kind), d_depth, int(w), int(h), int(B), C.byref(noise), d_depth_out, d_ir_out, stream))

    def scale(self, s):
        """HandTracker::scale (handtrack.h:591): both models of every slot grow by the factor s."""
        self._chk(self.L.ht_scale(self.h, float(s)))

    def slowfit(self, B, hold=0, refpose=None, steps=6, select_rb=-1, spoint=None, rbpoint=None, crays=None):
        """HandTracker::slowfit (handtrack.h:786-821) on the handmodel of slots [0,B) with the points of the last stage_prepare."""
        ref = None if refpose is None else _c(refpose, np.float32)
        sp = None if spoint is None else _c(spoint, np.float32); rp = None if rbpoint is None else _c(rbpoint, np.float32)
        cr = None if crays is None else _c(crays, np.float32)
        self._chk(self.L.ht_slowfit(self.h, int(B), int(hold), None if ref is None else _f(ref), int(steps), int(select_rb), None if sp is None else _f(sp), None if rp is None else _f(rp),
                                    None if cr is None else _f(cr), 0 if cr is None else int(cr.reshape(-1, 8, 4).shape[1])))

    def cnn_train(self, inputs, targets, alpha=0.001):
        """CNN::Train (cnn.h:558-580) sample after sample; returns the per-sample mean squared errors."""
        x = _c(inputs, np.float32).reshape(-1, CNN_IN); t = _c(targets, np.float32).reshape(-1, CNN_OUT)
        mse = np.zeros(x.shape[0], np.float32)
        self._chk(self.L.ht_cnn_train(self.h, _f(x), _f(t), x.shape[0], float(alpha), _f(mse)))
        return mse

    def cnn_train_dev(self, d_inputs, d_targets, n_pool, order=None, n_steps=None, alpha=0.001, d_mse=None, stream=None):
        """ht_cnn_train_dev: CNN::Train on device pools (inputs [n_pool,4096], targets [n_pool,2304]); step k uses sample order[k] (a host array of
        indices, checked before anything runs), or sample k without an order.  d_mse [n_steps] optional.  Asynchronous on `stream`."""
        o = None if order is None else np.ascontiguousarray(order, np.int32)
        n = (len(o) if o is not None else int(n_pool)) if n_steps is None else int(n_steps)
        if o is not None and len(o) < n:
            raise ValueError("order holds fewer than n_steps indices")
        self._chk(self.L.ht_cnn_train_dev(self.h, d_inputs, d_targets, int(n_pool), None if o is None else _i(o), n, float(alpha), d_mse, stream))

    @staticmethod
    def _side(side):
        side = int(side)
        if side not in (64, 128):
            raise ValueError("CNN input side must be 64 or 128")
        return side

    def cnn_train_batch(self, inputs, targets, batch, alpha=0.001, side=64):
        """ht_cnn_train_batch / _sized: mini-batch steps w' = w - alpha * SUM_b g_b(w) (a sum, not a mean) over the samples in order, `batch` per step (the
        remainder forms a last, smaller step); returns the per-sample losses at their step's weights.  side = 128 trains the 128x128-input net
        (inputs [n,16384])."""
        side = self._side(side)
        x = _c(inputs, np.float32).reshape(-1, side * side); t = _c(targets, np.float32).reshape(-1, CNN_OUT)
        mse = np.zeros(x.shape[0], np.float32)
        if side == 64:
            self._chk(self.L.ht_cnn_train_batch(self.h, _f(x), _f(t), x.shape[0], int(batch), float(alpha), _f(mse)))
        else:
            self._chk(self.L.ht_cnn_train_batch_sized(self.h, side, _f(x), _f(t), x.shape[0], int(batch), float(alpha), _f(mse)))
        return mse

    def cnn_train_batch_dev(self, d_inputs, d_targets, n_pool, batch, order=None, n_steps=None, alpha=0.001, d_mse=None, stream=None, side=64):
        """ht_cnn_train_batch_dev / _sized_dev: mini-batch steps on device pools (inputs [n_pool, side*side]); step k trains on samples
        order[k*batch:(k+1)*batch] (a host array, checked before anything runs), or k*batch + b without an order.  d_mse [n_steps*batch] optional.
        Asynchronous on `stream`."""
        side = self._side(side)
        o = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        batch = int(batch)
        n = ((len(o) if o is not None else int(n_pool)) // max(batch, 1)) if n_steps is None else int(n_steps)
        if o is not None and len(o) < n * batch:
            raise ValueError("order holds fewer than n_steps * batch indices")
        if side == 64:
            self._chk(self.L.ht_cnn_train_batch_dev(self.h, d_inputs, d_targets, int(n_pool), None if o is None else _i(o), n, batch, float(alpha), d_mse, stream))
        else:
            self._chk(self.L.ht_cnn_train_batch_sized_dev(self.h, side, d_inputs, d_targets, int(n_pool), None if o is None else _i(o), n, batch, float(alpha), d_mse, stream))

    def cnn_train_batch_buffers(self, n, side=64):
        """ht_debug_train_batch_buffers / _sized: the per-sample tensors of the latest mini-batch step of that net (n = its sample count): a3 [n,16,15,15],
        a6 [n,2304], a8 [n,2048], e9 [n,2304], e7 [n,2048], e6 [n,2304], e3 [n,16,15,15] (conv2's backward, summed over its groups); at side 128
        a3 / e3 [n,16,31,31] and a6 / e6 [n,12544]."""
        n = int(n); side = self._side(side)
        p2, n6 = (15, 2304) if side == 64 else (31, 12544)
        shapes = (("a3", (n, 16, p2, p2)), ("a6", (n, n6)), ("a8", (n, 2048)), ("e9", (n, 2304)), ("e7", (n, 2048)), ("e6", (n, n6)), ("e3", (n, 16, p2, p2)))
        out = {k: np.empty(sh, np.float32) for k, sh in shapes}
        if side == 64:
            self._chk(self.L.ht_debug_train_batch_buffers(self.h, n, *[_f(out[k]) for k, _ in shapes]))
        else:
            self._chk(self.L.ht_debug_train_batch_buffers_sized(self.h, side, n, *[_f(out[k]) for k, _ in shapes]))
        return out

    # -- the gradient as a buffer and the optimiser steps over it (ht_cnn_grad_* / ht_cnn_opt_*, csrc/ht_optim.hip)
    def _count(self, side):
        return CNNB_COUNT if self._side(side) == 64 else CNNB128_COUNT

    def cnn_grad_batch(self, inputs, targets, accumulate=False, side=64):
        """ht_cnn_grad_batch_sized: G = (accumulate ? G : 0) + SUM_b g_b(w) over the samples (at most 256), the weights untouched; returns their losses."""
        side = self._side(side)
        x = _c(inputs, np.float32).reshape(-1, side * side); t = _c(targets, np.float32).reshape(-1, CNN_OUT)
        mse = np.zeros(x.shape[0], np.float32)
        self._chk(self.L.ht_cnn_grad_batch_sized(self.h, side, _f(x), _f(t), x.shape[0], int(bool(accumulate)), _f(mse)))
        return mse

    def cnn_grad_batch_dev(self, d_inputs, d_targets, n_pool, batch, order=None, accumulate=False, d_mse=None, stream=None, side=64):
        """ht_cnn_grad_batch_sized_dev: the same on device pools, samples order[0:batch] (a host array) or 0..batch-1; asynchronous on `stream`."""
        side = self._side(side)
        o = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        if o is not None and len(o) < int(batch):
            raise ValueError("order holds fewer than batch indices")
        self._chk(self.L.ht_cnn_grad_batch_sized_dev(self.h, side, d_inputs, d_targets, int(n_pool), None if o is None else _i(o), int(batch), int(bool(accumulate)), d_mse, stream))

    def cnn_grad_get(self, side=64):
        """ht_cnn_grad_get_sized: G in .cnnb order"""
        g = np.empty(self._count(side), np.float32)
        self._chk(self.L.ht_cnn_grad_get_sized(self.h, int(side), _f(g), g.size))
        return g

    def cnn_grad_set(self, g, side=64):
        """ht_cnn_grad_set_sized"""
        g = _c(g, np.float32).reshape(-1)
        side = self._side(side)
        self._chk(self.L.ht_cnn_grad_set_sized(self.h, side, _f(g), g.size))

    def cnn_grad_ptr(self, side=64):
        """ht_cnn_grad_ptr_sized: (device address of G, its length)"""
        p = C.c_void_p(); n = C.c_size_t()
        side = self._side(side)
        self._chk(self.L.ht_cnn_grad_ptr_sized(self.h, side, C.byref(p), C.byref(n)))
        return p.value, n.value

    def cnn_opt_step(self, opt, stream=None, side=64):
        """ht_cnn_opt_step_sized_dev: one step of the optimiser `opt` (an Opt) over all weights of the net from its G; asynchronous on `stream`."""
        side = self._side(side)
        self._chk(self.L.ht_cnn_opt_step_sized_dev(self.h, side, C.byref(opt), stream))

    def cnn_opt_reset(self, side=64):
        """ht_cnn_opt_reset_sized: m = v = 0, t = 0"""
        side = self._side(side)
        self._chk(self.L.ht_cnn_opt_reset_sized(self.h, side))

    def cnn_opt_state(self, side=64):
        """ht_cnn_opt_state_get_sized: (m, v, t); a moment no step has needed yet is zeros"""
        n = self._count(side)
        m = np.empty(n, np.float32); v = np.empty(n, np.float32); t = C.c_int()
        self._chk(self.L.ht_cnn_opt_state_get_sized(self.h, int(side), _f(m), _f(v), n, C.byref(t)))
        return m, v, t.value

    def cnn_opt_set_state(self, m=None, v=None, t=0, side=64):
        """ht_cnn_opt_state_set_sized: m and / or v (None: left as it is) and t"""
        side = self._side(side)
        m = None if m is None else _c(m, np.float32).reshape(-1); v = None if v is None else _c(v, np.float32).reshape(-1)
        self._chk(self.L.ht_cnn_opt_state_set_sized(self.h, side, None if m is None else _f(m), None if v is None else _f(v), self._count(side), int(t)))

    def cnn_opt_last(self, side=64):
        """ht_cnn_opt_last_sized: (gradient norm, clip factor) of the latest step; (-1, 1) when it did not clip"""
        nrm = C.c_double(); c = C.c_float()
        side = self._side(side)
        self._chk(self.L.ht_cnn_opt_last_sized(self.h, side, C.byref(nrm), C.byref(c)))
        return nrm.value, np.float32(c.value)

    def cnn_train_opt_dev(self, d_inputs, d_targets, n_pool, batch, opt, accum=1, order=None, n_steps=None, d_mse=None, stream=None, side=64):
        """ht_cnn_train_opt_sized_dev: n_steps optimiser steps, each after `accum` gradient calls of `batch` samples; order holds n_steps * accum * batch
        indices (a host array, checked before anything runs).  Exactly that sequence of cnn_grad_batch_dev and cnn_opt_step calls."""
        side = self._side(side)
        o = None if order is None else np.ascontiguousarray(order, np.int32).reshape(-1)
        batch = int(batch); accum = int(accum); per = max(batch, 1) * max(accum, 1)
        n = ((len(o) if o is not None else int(n_pool)) // per) if n_steps is None else int(n_steps)
        if o is not None and len(o) < n * per:
            raise ValueError("order holds fewer than n_steps * accum * batch indices")
        self._chk(self.L.ht_cnn_train_opt_sized_dev(self.h, side, d_inputs, d_targets, int(n_pool), None if o is None else _i(o), n, batch, accum, C.byref(opt), d_mse, stream))

    # -- training samples on the device
    def expected_cnn_batch(self, poses, cams, segment_frame=False, side=64):
        """GatherHandExpectedCNN (handtrack.h:160-173) for a batch on the device: poses [B,nb,7], tile cameras [B,12] -> (expected [B,2304],
        image_points [B,8,2], vals [B,16]); segment_frame: train-cnn's compress first (HT_LABELS_SEGMENT_FRAME); side = 128: the cameras are those of
        128x128 tiles (HT_LABELS_SIDE128)."""
        poses = _c(poses, np.float32).reshape(-1, self.nb, POSE); B = poses.shape[0]
        cams = _c(cams, np.float32).reshape(B, CAM)
        e = np.empty((B, CNN_OUT), np.float32); ip = np.empty((B, 8, 2), np.float32); v = np.empty((B, 16), np.float32)
        flags = self._label_flags(segment_frame, side)
        self._chk(self.L.ht_expected_cnn_batch(self.h, _f(poses), _f(cams), B, flags, _f(e), _f(ip), _f(v)))
        return e, ip, v

    def _label_flags(self, segment_frame, side):
        return (LABELS_SEGMENT_FRAME if segment_frame else 0) | (LABELS_SIDE128 if self._side(side) == 128 else 0)

    def expected_cnn_dev(self, d_poses, d_cams, B, d_expected, d_image_points=None, d_vals=None, segment_frame=False, stream=None, side=64):
        """ht_expected_cnn_dev: device pointers (poses [B,nb,7], cams [B,12] -> expected [B,2304], image_points [B,8,2] / vals [B,16] or None), asynchronous on `stream`."""
        flags = self._label_flags(segment_frame, side)
        self._chk(self.L.ht_expected_cnn_dev(self.h, d_poses, d_cams, int(B), flags, d_expected, d_image_points, d_vals, stream))

    def cnn_input_dev(self, d_tiles, d_cams, B, d_cnn_in, stream=None, side=64):
        """ht_cnn_input_dev / _sized_dev: the net's input (handtrack.h:700) of B side x side tiles u16[B,side*side] with cameras [B,12] -> float
        [B,side*side], asynchronous on `stream`."""
        side = self._side(side)
        if side == 64:
            self._chk(self.L.ht_cnn_input_dev(self.h, d_tiles, d_cams, int(B), d_cnn_in, stream))
        else:
            self._chk(self.L.ht_cnn_input_sized_dev(self.h, side, d_tiles, d_cams, int(B), d_cnn_in, stream))

    def cnn_get_weights(self, side=64):
        """ht_cnn_get_weights / _sized: the weights of either net in .cnnb order (CNN::saveb)."""
        side = self._side(side)
        w = np.empty(CNNB_COUNT if side == 64 else CNNB128_COUNT, np.float32)
        if side == 64:
            self._chk(self.L.ht_cnn_get_weights(self.h, _f(w), w.size))
        else:
            self._chk(self.L.ht_cnn_get_weights_sized(self.h, side, _f(w), w.size))
        return w

    def cnn_train_buffers(self):
        """ht_debug_train_buffers: what the latest training step left behind, as named views of two arrays: the layer outputs a1 [16,60,60],
        a3 [16,15,15], a5 [64,12,12], a6 [2304], a8 [2048], the errors e9 [2304], e7 [2048], e6 [2304], conv2's backward as partial sums
        part3 [16,3600] (one per group of four output channels) and the soft-max blocks' sums of squares sqp [9]."""
        act = np.empty(sum(n for _, n, _ in TRAIN_ACT), np.float32); err = np.empty(sum(n for _, n, _ in TRAIN_ERR), np.float32)
        self._chk(self.L.ht_debug_train_buffers(self.h, _f(act), act.size, _f(err), err.size))
        out = {}
        for buf, table in ((act, TRAIN_ACT), (err, TRAIN_ERR)):
            o = 0
            for name, n, shape in table:
                if name:
                    out[name] = buf[o:o + n].reshape(shape)
                o += n
        return out


def kpfit_default(**kw):
    """ht_kpfit_default's options (6 steps, FLT_MAX, radius 0.01, ray force 100000, no flags) with the given fields replaced; keep_momenta=True sets the flag."""
    o = KpFit()
    if load().ht_kpfit_default(C.byref(o)) != HT_OK:
        raise HTError("ht_kpfit_default failed")
    if kw.pop("keep_momenta", False):
        o.flags |= KPFIT_KEEP_MOMENTA
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def sensor_noise_default(kind, depth_scale=0.001, far=4.0, **kw):
    """ht_sensor_noise_default: a plausible SensorNoise for camera `kind` (figures reasoned from data sheets, never measured against a camera), with the fields
    in kw changed.  ValueError for what the library refuses.  No context, no device."""
    n = SensorNoise()
    if load().ht_sensor_noise_default(int(kind), float(depth_scale), float(far), C.byref(n)) != HT_OK:
        raise ValueError("ht_sensor_noise_default refuses kind %d, depth_scale %g, far %g" % (kind, depth_scale, far))
    return n.but(**kw) if kw else n


def sensor_out_dims(kind, w, h, max_width=320):
    """ht_sensor_out_dims: (w_out, h_out) of a filtered frame; ValueError for what the filters refuse on sizes alone.  No context, no device."""
    wo, ho = C.c_int(0), C.c_int(0)
    if load().ht_sensor_out_dims(int(kind), int(w), int(h), int(max_width), C.byref(wo), C.byref(ho)) != HT_OK:
        raise ValueError("ht_sensor_out_dims refuses kind %d, %dx%d, max_width %d" % (kind, w, h, max_width))
    return wo.value, ho.value


def comm_available():
    """True when RCCL can be loaded on this host (ht_comm_available): agreed on by all ranks before any of them calls comm_init."""
    return load().ht_comm_available() == 1


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 makes it, the host program distributes it)."""
    L = load()
    buf = C.create_string_buffer(128)
    if L.ht_comm_unique_id(C.cast(buf, C.c_void_p)) != 0:
        raise HTError("ht_comm_unique_id failed (RCCL not available?)")
    return buf.raw


def expected_cnn(pose, cam):
    """GatherHandExpectedCNN(pose, camsub(cam, 4)).cnn_expected (handtrack.h:160-173), host only."""
    out = np.empty(CNN_OUT, np.float32)
    r = load().ht_expected_cnn(_f(_c(pose, np.float32)), _f(_c(cam, np.float32)), _f(out))
    if r != 0:
        raise HTError("ht_expected_cnn failed with status %d" % r)
    return out


def joint_degrees(coords):
    """Joint coordinates as angles in the reference's degrees: 2 asin(c) 180 / 3.14 (its 3.14; a host-side convenience)."""
    return 2.0 * np.arcsin(np.clip(np.asarray(coords, np.float64), -1.0, 1.0)) * 180.0 / 3.14


def model_joint_limits(path, hand_tweaks=True):
    """(lo [nj,3], hi [nj,3], swapped bool[nj]) of a model file's joint coordinates (ht_model_joint_limits; host only, no GPU)."""
    m = HostModel(path, hand_tweaks)
    try:
        return m.joint_limits()
    finally:
        m.close()


class HostModel:
    """A hand model that is not being tracked (ht_model_*, host only): the mesh ray cast's definition and its frames."""

    def __init__(self, path, hand_tweaks=True):
        self.L = load()
        self.m = C.c_void_p()
        r = self.L.ht_model_open(str(path).encode(), 1 if hand_tweaks else 0, C.byref(self.m))
        if r:
            self.L.ht_model_error.restype = C.c_char_p
            msg = self.L.ht_model_error(self.m).decode(); self.close()
            raise HTError("ht_model_open(%s): %s" % (path, msg))
        nb, nj = C.c_int(), C.c_int()
        self.L.ht_model_counts(self.m, C.byref(nb), C.byref(nj))
        self.nb, self.nj = nb.value, nj.value

    def close(self):
        if self.m:
            self.L.ht_model_close(self.m); self.m = C.c_void_p()

    def scale(self, s):
        if self.L.ht_model_scale(self.m, float(s)):
            raise HTError("ht_model_scale: bad argument")

    def mirror(self):
        """the left hand of this model, in place (ht_model_mirror): sign flips of the stored arrays, twice is the identity"""
        if self.L.ht_model_mirror(self.m):
            raise HTError("ht_model_mirror: bad argument")

    def body(self, body):
        """(verts [n,3], tris int32[t,3], planes [p,4], com [3], rest pose [7]) of a body's hull"""
        nv, nt, npl = C.c_int(), C.c_int(), C.c_int()
        com = np.empty(3, np.float32); rest = np.empty(7, np.float32)
        self.L.ht_model_body(self.m, int(body), C.byref(nv), C.byref(nt), C.byref(npl), _f(com), _f(rest))
        v = np.empty((nv.value, 3), np.float32); t = np.empty((nt.value, 3), np.int32); p = np.empty((npl.value, 4), np.float32)
        self.L.ht_model_body_mesh(self.m, int(body), _f(v), _i(t))
        self.L.ht_model_body_planes(self.m, int(body), _f(p), None)
        return v, t, p, com, rest

    def sdmesh_planes(self, body):
        """the PolyPlane [t,4] of every triangle of body's subdivision mesh, as the mesh ray cast reads it"""
        n = C.c_int()
        self.L.ht_model_body_sdmesh(self.m, int(body), C.byref(n), None)
        p = np.empty((n.value // 3, 4), np.float32)
        self.L.ht_model_body_planes(self.m, int(body), None, _f(p))
        return p

    def hitcheck(self, poses, v0, v1):
        """(impact[3], normal[3], body) of the segment v0 -> v1 against the hulls at centre-of-mass poses [nb,7] (ht_model_hitcheck)"""
        poses = _c(poses, np.float32); v0 = _c(v0, np.float32); v1 = _c(v1, np.float32)
        imp = np.empty(3, np.float32); nrm = np.empty(3, np.float32); b = C.c_int()
        if self.L.ht_model_hitcheck(self.m, _f(poses), _f(v0), _f(v1), _f(imp), _f(nrm), C.byref(b)):
            raise HTError("ht_model_hitcheck: bad argument")
        return imp, nrm, b.value

    def joint_limits(self):
        lo = np.empty((self.nj, 3), np.float32); hi = np.empty((self.nj, 3), np.float32); sw = np.zeros(self.nj, np.int32)
        if self.L.ht_model_joint_limits(self.m, _f(lo), _f(hi), _i(sw)):
            raise HTError("ht_model_joint_limits: bad argument")
        return lo, hi, sw.astype(bool)

    def sdmesh(self, body):
        """corner positions [3 t, 3] of body's subdivision mesh, in the bone's rig frame"""
        n = C.c_int()
        self.L.ht_model_body_sdmesh(self.m, int(body), C.byref(n), None)
        v = np.empty((n.value, 3), np.float32)
        self.L.ht_model_body_sdmesh(self.m, int(body), None, _f(v))
        return v

    def com(self, body):
        c = np.empty(3, np.float32)
        self.L.ht_model_body(self.m, int(body), None, None, None, _f(c), None)
        return c

    def hitcheck_mesh(self, poses, v0, v1):
        """(impact[3], normal[3], body, triangle) of the segment v0 -> v1 against the subdivision surface at poses [nb,7]"""
        poses = _c(poses, np.float32); v0 = _c(v0, np.float32); v1 = _c(v1, np.float32)
        imp = np.empty(3, np.float32); nrm = np.empty(3, np.float32); b, t = C.c_int(), C.c_int()
        if self.L.ht_model_hitcheck_mesh(self.m, _f(poses), _f(v0), _f(v1), _f(imp), _f(nrm), C.byref(b), C.byref(t)):
            raise HTError("ht_model_hitcheck_mesh: bad argument")
        return imp, nrm, b.value, t.value

    def render_mesh(self, poses, cam, w, h, far=4.0, pixel_offset=0.0):
        """one frame of the definition: (depth u16[h,w], body int8[h,w])"""
        poses = _c(poses, np.float32); cam = _c(cam, np.float32)
        depth = np.empty((int(h), int(w)), np.uint16); body = np.empty((int(h), int(w)), np.int8)
        if self.L.ht_model_render_mesh(self.m, _f(poses), _f(cam), int(w), int(h), float(far), float(pixel_offset), depth.ctypes.data_as(C.POINTER(C.c_uint16)), body.ctypes.data_as(C.POINTER(C.c_int8))):
            raise HTError("ht_model_render_mesh: bad argument")
        return depth, body

    def raster_mesh(self, poses, cam, w, h, far=4.0, pixel_offset=0.0):
        """one frame of the rasteriser's definition (ht_model_raster_mesh): (depth u16[h,w], body int8[h,w])"""
        poses = _c(poses, np.float32); cam = _c(cam, np.float32)
        depth = np.empty((int(h), int(w)), np.uint16); body = np.empty((int(h), int(w)), np.int8)
        if self.L.ht_model_raster_mesh(self.m, _f(poses), _f(cam), int(w), int(h), float(far), float(pixel_offset), depth.ctypes.data_as(C.POINTER(C.c_uint16)), body.ctypes.data_as(C.POINTER(C.c_int8))):
            raise HTError("ht_model_raster_mesh: bad argument")
        return depth, body

    def raster_scene(self, poses, cam, w, h, hands=None, far=4.0, pixel_offset=0.0, bg=None, in_place=False):
        """one frame of the scene's definition (ht_model_raster_scene): poses [H,nb,7], hands u8[H] or None, bg u16[h,w] or None ->
        (depth u16[h,w], hand int8[h,w], body int8[h,w], visible int32[H]).  in_place: bg itself is composed and returned as depth."""
        poses = _c(poses, np.float32); H = poses.shape[0]; cam = _c(cam, np.float32)
        hands = None if hands is None else _c(hands, np.uint8).reshape(H)
        bg = None if bg is None else _c(bg, np.uint16).reshape(int(h), int(w))
        depth = bg if (in_place and bg is not None) else np.empty((int(h), int(w)), np.uint16)
        hand = np.empty((int(h), int(w)), np.int8); body = np.empty((int(h), int(w)), np.int8); visible = np.empty(H, np.int32)
        u16p, i8p = C.POINTER(C.c_uint16), C.POINTER(C.c_int8)
        r = self.L.ht_model_raster_scene(self.m, _f(poses), hands.ctypes.data_as(C.POINTER(C.c_uint8)) if hands is not None else None, H, _f(cam), int(w), int(h), float(far), float(pixel_offset),
                                         bg.ctypes.data_as(u16p) if bg is not None else None, depth.ctypes.data_as(u16p), hand.ctypes.data_as(i8p), body.ctypes.data_as(i8p), _i(visible))
        if r:
            raise HTError("ht_model_raster_scene: status %d" % r)
        return depth, hand, body, visible


Model = HostModel      # the name the C ABI uses (ht_model): Model.mirror() is ht_model_mirror
