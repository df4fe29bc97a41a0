"""ctypes binding of the C ABI in include/ccal.h.

Fails loudly when the HIP library has not been built: there is no CPU fallback in the product.
"""
from __future__ import annotations

import ctypes as C
import os

PMAX = 10
MAX_CAMS = 8
KMAX = 128

OK, ERR_INVALID_ARG, ERR_HIP, ERR_NONFINITE, ERR_NOT_PD, ERR_NO_CONVERGENCE, ERR_UNSUPPORTED, ERR_NO_MEMORY, NO_RESULT = range(9)
STATUS_NAMES = ["CCAL_OK", "CCAL_ERR_INVALID_ARG", "CCAL_ERR_HIP", "CCAL_ERR_NONFINITE", "CCAL_ERR_NOT_PD",
                "CCAL_ERR_NO_CONVERGENCE", "CCAL_ERR_UNSUPPORTED", "CCAL_ERR_NO_MEMORY", "CCAL_NO_RESULT"]
METHOD_GN, METHOD_LM = 0, 1
TRANSPORT_NONE, TRANSPORT_RCCL, TRANSPORT_INPROC = 0, 1, 2
MULTI_MAX_DEVICES = 16
PIX_U8, PIX_U16 = 0, 1                          # ccal_pixel_type
TAG_OK, TAG_OUTSIDE, TAG_LOW_CONTRAST, TAG_BORDER, TAG_NO_CODE = range(5)        # ccal_tag_reason
QUAD_MAX_OUT_EDGES = 8                          # CCAL_QUAD_MAX_OUT_EDGES
QUAD_FLAG_CUT = 1                               # bit 0 of ccal_propose_quads_*'s flags_out: an out-edge list was cut

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int32)
_lp = C.POINTER(C.c_int64)
_bp = C.POINTER(C.c_uint8)
_up = C.POINTER(C.c_uint64)


class ProblemDesc(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("model", _ip), ("width", _dp), ("height", _dp),
        ("xy_same_focal", C.c_int32), ("n_slots", C.c_int32), ("n_obs", C.c_int32),
        ("obs_cam", _ip), ("obs_slot", _ip), ("obs_offsets", _lp),
        ("p3d_x", _fp), ("p3d_y", _fp), ("p3d_z", _fp), ("p2d_u", _fp), ("p2d_v", _fp),
        ("huber_delta", C.c_double),
    ]


class SolverOpts(C.Structure):
    _fields_ = [
        ("method", C.c_int32), ("max_iterations", C.c_int32),
        ("min_abs_error_decrease", C.c_double), ("min_rel_error_decrease", C.c_double), ("min_error", C.c_double),
        ("lm_initial_radius", C.c_double), ("lm_min_diagonal", C.c_double), ("lm_max_diagonal", C.c_double),
        ("verbose", C.c_int32), ("timeout_s", C.c_int32),
        ("error_metric", C.c_int32), ("reserved_", C.c_int32),
    ]


ERROR_SQUARED_NORM, ERROR_NORM = 0, 1          # ccal_error_metric (ccal_solver_opts.error_metric)


class Report(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("iterations", C.c_int32), ("lm_accepted", C.c_int32), ("lm_rejected", C.c_int32),
        ("initial_cost", C.c_double), ("final_cost", C.c_double), ("solve_ms", C.c_double),
        ("lm_spec_hits", C.c_int32), ("lm_spec_misses", C.c_int32),
    ]


class CovReport(C.Structure):             # ccal_cov_report
    _fields_ = [("status", C.c_int32), ("bad_slot", C.c_int32), ("dof", C.c_int64), ("n_free", C.c_int32), ("n_posed", C.c_int32),
                ("cost", C.c_double), ("sigma2", C.c_double), ("leverage_sum", C.c_double), ("reserved_", C.c_int32 * 4)]


class ModelConventions(C.Structure):
    _fields_ = [("kb4_small_radius", C.c_double), ("dist_lo", (C.c_double * 5) * 4), ("dist_hi", (C.c_double * 5) * 4),
                ("unproject_small_radius", C.c_double), ("ocv5_order", C.c_int32 * 5), ("reserved_", C.c_int32)]


class DetectTagsOpts(C.Structure):          # ccal_detect_tags_opts: every field is the stage parameter of that name
    _fields_ = [
        ("step", C.c_int32), ("nms_radius", C.c_int32), ("min_response", C.c_int64), ("rel_q10", C.c_int32), ("cand_cap", C.c_int32),
        ("half_win", C.c_int32), ("max_iterations", C.c_int32), ("eps", C.c_double),
        ("merge_radius", C.c_double),
        ("min_side", C.c_double), ("max_side", C.c_double), ("max_side_ratio", C.c_double), ("offset", C.c_double),
        ("edge_min_contrast", C.c_double), ("edge_samples", C.c_int32), ("quad_cap", C.c_int32),
        ("border", C.c_int32), ("cell_samples", C.c_int32), ("tag_min_contrast", C.c_double),
        ("max_border_errors", C.c_int32), ("max_hamming", C.c_int32),
        ("tag_cap", C.c_int32), ("reserved_", C.c_int32),
    ]


# bits of ccal_detect_tags_*'s flags_out: an out-edge list was cut; more candidates than cand_cap, quads than quad_cap, tags than tag_cap
TAGS_FLAG_CUT, TAGS_FLAG_CAND_CAP, TAGS_FLAG_QUAD_CAP, TAGS_FLAG_TAG_CAP = 1, 2, 4, 8


class DetectCheckerboardsOpts(C.Structure):          # ccal_detect_checkerboards_opts: every field is the stage parameter of that name
    _fields_ = [
        ("step", C.c_int32), ("nms_radius", C.c_int32), ("min_response", C.c_int64), ("rel_q10", C.c_int32), ("cand_cap", C.c_int32),
        ("half_win", C.c_int32), ("max_iterations", C.c_int32), ("eps", C.c_double),
        ("cols", C.c_int32), ("rows", C.c_int32), ("reserved_", C.c_int64),
    ]


# the checkerboard assembly's limits (CCAL_BOARD_*) and the bits of its flags_out: more candidates than cand_cap (the fused call
# only), more than BOARD_MAX_KEPT rows kept after the screen - no board
BOARD_MIN_SIDE, BOARD_MAX_SIDE, BOARD_MAX_ROWS, BOARD_MAX_KEPT = 2, 20, 4096, 512
BOARD_FLAG_CAND_CAP, BOARD_FLAG_KEPT_LIMIT = 1, 2

TARGET_CHECKERBOARD, TARGET_APRILGRID = 0, 1    # ccal_target_kind


class RenderTarget(C.Structure):          # ccal_render_target: one struct for both kinds of target
    _fields_ = [
        ("kind", C.c_int32), ("cols", C.c_int32), ("rows", C.c_int32), ("reserved_", C.c_int32), ("square", C.c_double),
        ("tag_size", C.c_double), ("tag_spacing", C.c_double),
        ("tag_rows", C.c_int32), ("tag_cols", C.c_int32), ("first_id", C.c_int32), ("family_bits", C.c_int32),
        ("n_codes", C.c_int32), ("border", C.c_int32), ("codes", _up),
    ]


class RenderOpts(C.Structure):            # ccal_render_opts
    _fields_ = [("supersample", C.c_int32), ("reserved_", C.c_int32), ("black", C.c_double), ("white", C.c_double),
                ("background", C.c_double), ("margin", C.c_double)]


class PhotoOpts(C.Structure):             # ccal_photo_opts: the photometric stage; ccal_photo_set_defaults switches everything off
    _fields_ = [("blur_sigma", C.c_double), ("vignette", C.c_double), ("gain", C.c_double), ("noise_read", C.c_double),
                ("noise_shot", C.c_double), ("seed", C.c_uint64), ("first_index", C.c_int64)]


PHOTO_MAX_RADIUS = 16                     # CCAL_PHOTO_MAX_RADIUS


class NormalizeOpts(C.Structure):         # ccal_normalize_opts: local contrast normalisation; ccal_normalize_set_defaults: 16, 0, 4.0, 64.0
    _fields_ = [("radius", C.c_int32), ("reserved_", C.c_int32), ("min_sigma", C.c_double), ("amp", C.c_double)]


NORMALIZE_MAX_RADIUS = 32                 # CCAL_NORMALIZE_MAX_RADIUS


class GreyOpts(C.Structure):              # ccal_grey_opts: the grey stage; ccal_grey_set_defaults: 1; 19595, 38470, 7471
    _fields_ = [("bin", C.c_int32), ("w_r", C.c_int32), ("w_g", C.c_int32), ("w_b", C.c_int32)]


# ccal_pixel_layout: what a source pixel of ccal_grey_dev is
(LAYOUT_GREY, LAYOUT_RGB, LAYOUT_BGR, LAYOUT_RGBA, LAYOUT_BGRA,
 LAYOUT_BAYER_RGGB, LAYOUT_BAYER_BGGR, LAYOUT_BAYER_GRBG, LAYOUT_BAYER_GBRG) = range(9)

ALLREDUCE_FN =C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)

LIB_PATH = os.environ.get("CCAL_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libccal_hip.so")

# every symbol include/ccal.h declares: (name, restype, argtypes)
_vp = C.c_void_p
SYMBOLS = [
    ("ccal_ctx_create", C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    ("ccal_ctx_destroy", None, [_vp]),
    ("ccal_last_error", C.c_char_p, [_vp]),
    ("ccal_version", C.c_char_p, []),
    ("ccal_model_num_params", C.c_int, [C.c_int]),
    ("ccal_problem_create", C.c_int, [_vp, C.POINTER(ProblemDesc), C.POINTER(_vp)]),
    ("ccal_problem_destroy", None, [_vp]),
    ("ccal_set_defaults", C.c_int, [C.POINTER(SolverOpts)]),
    ("ccal_set_bounds", C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double]),
    ("ccal_clear_bounds", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_fix_param", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_unfix_param", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_apply_reference_bounds", C.c_int, [_vp]),
    ("ccal_disable_distortions", C.c_int, [_vp, C.c_int, _dp]),
    ("ccal_set_allreduce", C.c_int, [_vp, ALLREDUCE_FN, _vp]),
    ("ccal_set_rccl_comm", C.c_int, [_vp, _vp]),
    ("ccal_rccl_available", C.c_int, []),
    ("ccal_rccl_version", C.c_int, []),
    ("ccal_rccl_unique_id", C.c_int, [_vp]),
    ("ccal_rccl_comm_create", C.c_int, [_vp, C.c_int, C.c_int, _vp, C.POINTER(_vp)]),
    ("ccal_rccl_comm_destroy", C.c_int, [_vp]),
    ("ccal_rccl_comm_count", C.c_int, [_vp]),
    ("ccal_get_model_conventions", C.c_int, [_vp, C.POINTER(ModelConventions)]),
    ("ccal_set_model_conventions", C.c_int, [_vp, C.POINTER(ModelConventions)]),
    ("ccal_num_corners", C.c_int64, [_vp]),
    ("ccal_reduced_dim", C.c_int, [_vp]),
    ("ccal_block_dim", C.c_int, [_vp, C.c_int]),
    ("ccal_eff_num_params", C.c_int, [_vp, C.c_int]),
    ("ccal_jacobian_len", C.c_int64, [_vp]),
    ("ccal_eval", C.c_int, [_vp, _dp, _dp, _dp, C.c_int, _dp, _dp]),
    ("ccal_upload_params", C.c_int, [_vp, _dp, _dp, _dp]),
    ("ccal_download_params", C.c_int, [_vp, _dp, _dp, _dp]),
    ("ccal_eval_dev", C.c_int, [_vp, C.c_int, _vp, _vp]),
    ("ccal_sync", C.c_int, [_vp]),
    ("ccal_build_normal", C.c_int, [_vp, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp]),
    ("ccal_build_normal_dev", C.c_int, [_vp, C.c_double]),
    ("ccal_solve", C.c_int, [_vp, C.POINTER(SolverOpts), _dp, _dp, _dp, C.POINTER(Report)]),
    ("ccal_solve_dev", C.c_int, [_vp, C.POINTER(SolverOpts), C.POINTER(Report)]),
    ("ccal_solve_batch", C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(SolverOpts), C.POINTER(_dp), C.POINTER(_dp), C.POINTER(_dp),
                                   C.POINTER(Report)]),
    ("ccal_init_poses", C.c_int, [_vp, _dp, C.c_int, _dp, _ip]),
    ("ccal_rdh_batch", C.c_int, [_vp, C.c_int, _lp, _dp, C.POINTER(C.c_uint64), C.c_int, _dp, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp]),
    ("ccal_radial_distortion_homography", C.c_int, [_vp, _dp, C.c_int, C.c_uint64, C.c_int, _dp, _dp, _dp, _ip, _ip]),
    ("ccal_homography_to_focal", C.c_int, [_dp, _dp]),
    ("ccal_pnp_batch", C.c_int, [_vp, C.c_int, _lp, _dp, _dp, C.c_int, _dp, _ip, _dp]),
    ("ccal_refine_poses_batch", C.c_int, [_vp, C.c_int, _dp, C.c_double, C.c_int, _lp, _dp, _dp, C.c_int, C.POINTER(SolverOpts),
                                          _dp, _ip, _ip, _ip, _dp, _dp, _dp]),
    ("ccal_refine_rig_poses_batch", C.c_int, [_vp, C.c_int, _ip, _dp, _dp, C.c_double, C.c_int, _lp, _ip, _lp, _dp, _dp, C.c_int,
                                              C.POINTER(SolverOpts), _dp, _ip, _ip, _ip, _dp, _dp, _dp]),
    ("ccal_init_poses_division", C.c_int, [_vp, C.c_double, C.c_int, _dp, _ip]),
    ("ccal_pin_buffer", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    ("ccal_unpin_buffer", C.c_int, [C.c_void_p, C.c_void_p]),
    ("ccal_init_camera_extrinsic", C.c_int, [_dp, _dp, C.c_int, _dp, C.c_int, C.POINTER(Report)]),
    ("ccal_init_camera_extrinsic_opts", C.c_int, [_dp, _dp, C.c_int, _dp, C.c_int, C.POINTER(SolverOpts), C.POINTER(Report)]),
    ("ccal_se3_factor", C.c_int, [_dp, _dp, _dp, _dp, _dp]),
    # one process, several GPUs
    ("ccal_solve_sharded", C.c_int, [C.POINTER(_vp), C.c_int, C.POINTER(SolverOpts), _dp, C.POINTER(_dp), _dp, C.POINTER(Report)]),
    ("ccal_multi_create", C.c_int, [_ip, C.c_int, C.POINTER(_vp)]),
    ("ccal_multi_create_transport", C.c_int, [_ip, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("ccal_multi_rccl_ranks", C.c_int, [_vp]),
    ("ccal_create_last_error", C.c_char_p, []),
    ("ccal_partition_slots", C.c_int, [C.POINTER(ProblemDesc), C.c_int, _ip]),
    ("ccal_multi_destroy", None, [_vp]),
    ("ccal_multi_num_devices", C.c_int, [_vp]),
    ("ccal_multi_transport", C.c_int, [_vp]),
    ("ccal_multi_ctx", _vp, [_vp, C.c_int]),
    ("ccal_multi_last_error", C.c_char_p, [_vp]),
    ("ccal_multi_set_model_conventions", C.c_int, [_vp, C.POINTER(ModelConventions)]),
    ("ccal_multi_sync", C.c_int, [_vp]),
    ("ccal_multi_problem_create", C.c_int, [_vp, C.POINTER(ProblemDesc), C.POINTER(_vp)]),
    ("ccal_multi_problem_destroy", None, [_vp]),
    ("ccal_multi_problem_num_shards", C.c_int, [_vp]),
    ("ccal_multi_problem_shard", _vp, [_vp, C.c_int]),
    ("ccal_multi_problem_slot_range", C.c_int, [_vp, C.c_int, _ip, _ip]),
    ("ccal_multi_set_bounds", C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_double]),
    ("ccal_multi_clear_bounds", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_multi_fix_param", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_multi_unfix_param", C.c_int, [_vp, C.c_int, C.c_int]),
    ("ccal_multi_apply_reference_bounds", C.c_int, [_vp]),
    ("ccal_multi_disable_distortions", C.c_int, [_vp, C.c_int, _dp]),
    ("ccal_multi_init_poses", C.c_int, [_vp, _dp, C.c_int, _dp, _ip]),
    ("ccal_multi_upload_params", C.c_int, [_vp, _dp, _dp, _dp]),
    ("ccal_multi_eval_dev", C.c_int, [_vp, C.c_int, C.POINTER(_vp), C.POINTER(_vp)]),
    ("ccal_multi_solve", C.c_int, [_vp, C.POINTER(SolverOpts), _dp, _dp, _dp, C.POINTER(Report)]),
    ("ccal_multi_validation", C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    ("ccal_multi_reprojection_errors", C.c_int, [_vp, _dp, _dp, _dp, _dp, _lp]),
    ("ccal_convert_model", C.c_int, [C.c_void_p, C.c_int, _dp, C.c_int, _dp, C.c_double, C.c_double, C.c_int,
                                     C.POINTER(SolverOpts), C.POINTER(Report)]),
    # applying a calibration: points, undistortion maps, remap
    ("ccal_project_points", C.c_int, [_vp, C.c_int, _dp, C.c_int64, _dp, _dp, _bp]),
    ("ccal_unproject_points", C.c_int, [_vp, C.c_int, _dp, C.c_int64, _dp, _dp, _bp]),
    ("ccal_estimate_new_camera_matrix", C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, _dp]),
    ("ccal_undistort_map_create", C.c_int, [_vp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("ccal_undistort_map_from_host", C.c_int, [_vp, _fp, _fp, C.c_int, C.c_int, C.POINTER(_vp)]),
    ("ccal_undistort_map_download", C.c_int, [_vp, _fp, _fp]),
    ("ccal_undistort_map_destroy", None, [_vp]),
    ("ccal_remap", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    ("ccal_remap_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp]),
    # from pixels to detections: sub-pixel refinement of coarse corners
    ("ccal_refine_corners_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_int, C.c_int, C.c_double,
                                            _ip, _ip, _dp]),
    ("ccal_refine_corners_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_int, C.c_int, C.c_double,
                                          _ip, _ip, _dp]),
    # from pixels to detections: checkerboard-corner candidates of whole images
    ("ccal_detect_corners_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int,
                                            _ip, _ip, _ip, _lp]),
    ("ccal_detect_corners_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, C.c_int64, C.c_int, C.c_int,
                                          _ip, _ip, _ip, _lp]),
    # from pixels to detections: decoding tags in candidate quads
    ("ccal_decode_tags_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_int, C.c_int, _up, C.c_int, C.c_int,
                                         C.c_double, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _dp, _up, _dp]),
    ("ccal_decode_tags_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_int, C.c_int, _up, C.c_int, C.c_int,
                                       C.c_double, C.c_int, C.c_int, _ip, _ip, _ip, _ip, _dp, _up, _dp]),
    # from pixels to detections: proposing tag quads from corner candidates
    ("ccal_propose_quads_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_double, C.c_double, C.c_double,
                                           C.c_double, C.c_int, C.c_double, C.c_int, _ip, _ip, _ip, _dp]),
    ("ccal_propose_quads_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _lp, _dp, C.c_double, C.c_double, C.c_double,
                                         C.c_double, C.c_int, C.c_double, C.c_int, _ip, _ip, _ip, _dp]),
    # from pixels to detections: the four stages in one device-resident call
    ("ccal_detect_tags_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _up, C.c_int, C.POINTER(DetectTagsOpts),
                                         _ip, _ip, _ip, _ip, _dp, _dp, _ip, _ip]),
    ("ccal_detect_tags_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _up, C.c_int, C.POINTER(DetectTagsOpts),
                                       _ip, _ip, _ip, _ip, _dp, _dp, _ip, _ip]),
    # from pixels to detections: a complete checkerboard from corner candidates; images to boards in one device-resident call
    ("ccal_assemble_checkerboards_batch", C.c_int, [_vp, C.c_int, _lp, _dp, _dp, C.c_int, C.c_int, _ip, _dp, _ip, _ip, _ip]),
    ("ccal_detect_checkerboards_batch", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(DetectCheckerboardsOpts),
                                                  _ip, _dp, _ip, _ip]),
    ("ccal_detect_checkerboards_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(DetectCheckerboardsOpts),
                                                _ip, _dp, _ip, _ip]),
    # rendering calibration targets through the camera models
    ("ccal_render_set_defaults", C.c_int, [C.POINTER(RenderTarget), C.POINTER(RenderOpts)]),
    ("ccal_render_targets_batch", C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(RenderTarget),
                                            C.POINTER(RenderOpts), _vp]),
    ("ccal_render_targets_dev", C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(RenderTarget),
                                          C.POINTER(RenderOpts), _vp]),
    # the photometric stage: lens blur, vignetting, exposure and sensor noise
    ("ccal_photo_set_defaults", C.c_int, [C.POINTER(PhotoOpts)]),
    ("ccal_photo_tables", C.c_int, [C.POINTER(PhotoOpts), _ip, _dp, _dp]),
    ("ccal_photo_apply_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(PhotoOpts)]),
    ("ccal_render_photo_targets", C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(RenderTarget),
                                            C.POINTER(RenderOpts), C.POINTER(PhotoOpts), _vp]),
    ("ccal_render_photo_targets_dev", C.c_int, [_vp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.POINTER(RenderTarget),
                                                C.POINTER(RenderOpts), C.POINTER(PhotoOpts), _vp]),
    # local contrast normalisation ahead of the detectors
    ("ccal_normalize_set_defaults", C.c_int, [C.POINTER(NormalizeOpts)]),
    ("ccal_normalize_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(NormalizeOpts)]),
    ("ccal_grey_set_defaults", C.c_int, [C.POINTER(GreyOpts)]),
    ("ccal_grey_dev", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.POINTER(GreyOpts)]),
    ("ccal_reprojection_errors", C.c_int, [_vp, _dp, _dp, _dp, _dp]),
    ("ccal_validation", C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp]),
    # calibration uncertainty: covariances and leverage
    ("ccal_covariance", C.c_int, [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, C.POINTER(CovReport)]),
]

LEGACY_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libccal_hip_legacy.so")
_lib = None
_legacy = None


class CcalLibraryMissing(RuntimeError):
    pass


def _bind(path, mode):
    lib = C.CDLL(path, mode=mode)
    # A/B TOOLS ONLY: an OLDER build named through CCAL_LIB (tools/ab_build.py against a previous round's library) may lack the newest
    # entry points; CCAL_LIB_ALLOW_MISSING=1 binds what is there.  The product path never sets it: a missing export raises.
    tolerant = os.environ.get("CCAL_LIB_ALLOW_MISSING") == "1" and "CCAL_LIB" in os.environ
    for name, res, args in SYMBOLS:
        if tolerant and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)   # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    return lib


def load():
    """Load libccal_hip.so (built by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CcalLibraryMissing(
            f"{LIB_PATH} not found: the HIP engine is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C camera_intrinsic_calibration_rs_amd/csrc`).  There is no CPU fallback.")
    _lib = _bind(LIB_PATH, C.RTLD_GLOBAL)
    return _lib


def load_for_switches():
    """TEST / A-B INFRASTRUCTURE: the second build when a developer switch (any CCAL_* variable the product ignores) is set in the
    environment, else the product library.  Child processes of the tests call this after setting their switch."""
    keep = {"CCAL_LIB", "CCAL_RCCL_LIB", "CCAL_MULTI_TRANSPORT"}
    dev = any(k.startswith("CCAL_") and k not in keep and not k.startswith("CCAL_BENCH") for k in os.environ)
    return load_legacy() if dev else load()


def load_legacy():
    """TEST INFRASTRUCTURE: the second build of the library that still carries the superseded matrix-core kernels
    (-DCCAL_LEGACY_KERNELS: k_gram1, k_gram, k_schur<false>; CCAL_GRAM=mfma / CCAL_GENERAL_GRAM=mfma select them there) - the
    independent second implementation some parity tests hold the product kernels against.  engine.Context(lib=load_legacy())."""
    global _legacy
    if _legacy is None:
        if not os.path.exists(LEGACY_LIB_PATH):
            raise CcalLibraryMissing(f"{LEGACY_LIB_PATH} not found (make -C camera_intrinsic_calibration_rs_amd/csrc)")
        _legacy = _bind(LEGACY_LIB_PATH, C.RTLD_LOCAL)
    return _legacy
