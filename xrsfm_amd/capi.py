"""ctypes binding of the C-ABI in include/xrsfm_ba.h (the product path: HIP only).

There is deliberately no CPU fallback here: if the shared library is missing or
no HIP device is visible the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

_c_double_p = C.POINTER(C.c_double)
_c_int32_p = C.POINTER(C.c_int32)
_c_uint8_p = C.POINTER(C.c_uint8)


class CProblem(C.Structure):
    _fields_ = [
        ("n_cams", C.c_int32), ("n_points", C.c_int32), ("n_obs", C.c_int32), ("n_intr", C.c_int32),
        ("cam_q", _c_double_p), ("cam_t", _c_double_p), ("cam_const", _c_uint8_p), ("cam_intr", _c_int32_p),
        ("intr_model", _c_int32_p), ("intr_params", _c_double_p),
        ("points", _c_double_p), ("point_const", _c_uint8_p),
        ("obs_cam", _c_int32_p), ("obs_pt", _c_int32_p), ("obs_uv", _c_double_p),
    ]


class CPgProblem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("n_scales", C.c_int32), ("n_edges", C.c_int32), ("n_scale_costs", C.c_int32),
                ("rot_q", _c_double_p), ("pos", _c_double_p), ("scale", _c_double_p), ("pos_const", _c_uint8_p),
                ("scale_const", _c_uint8_p), ("scale_lower", _c_double_p), ("edge_a", _c_int32_p), ("edge_b", _c_int32_p),
                ("edge_sa", _c_int32_p), ("edge_sb", _c_int32_p), ("edge_q_mea", _c_double_p), ("edge_p_mea", _c_double_p),
                ("weight_o", C.c_double), ("sc_a", _c_int32_p), ("sc_b", _c_int32_p), ("sc_s12", _c_double_p)]


class CPgOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double), ("initial_radius", C.c_double), ("verbose", C.c_int32),
                ("bounds_active_set", C.c_int32)]


class CPgSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double), ("iterations", C.c_int32), ("n_successful", C.c_int32),
                ("n_unsuccessful", C.c_int32), ("termination", C.c_int32)]


class CTagProblem(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("frame_q", _c_double_p), ("frame_t", _c_double_p), ("n_tags", C.c_int32),
                ("tag_length", C.c_double), ("tag_corners", _c_double_p), ("tag_q", _c_double_p), ("tag_t", _c_double_p),
                ("scale", C.c_double), ("scale_lower", C.c_double), ("n_tag_obs", C.c_int32), ("tag_obs_tag", _c_int32_p),
                ("tag_obs_frame", _c_int32_p), ("tag_obs_xy", _c_double_p), ("n_points", C.c_int32), ("n_obs", C.c_int32),
                ("points", _c_double_p), ("obs_frame", _c_int32_p), ("obs_pt", _c_int32_p), ("obs_xy", _c_double_p)]


class CPoseOptions(C.Structure):
    _fields_ = [("max_error", C.c_double), ("confidence", C.c_double), ("min_inlier_ratio", C.c_double),
                ("min_num_trials", C.c_int32), ("max_num_trials", C.c_int32), ("seed", C.c_uint32)]


class CTwoViewOptions(C.Structure):
    _fields_ = [("confidence", C.c_double), ("max_iterations", C.c_int32), ("seed", C.c_uint32), ("min_matches", C.c_int32),
                ("max_depth", C.c_double), ("n_angles", C.c_int32), ("min_angle_rad", C.c_double * 4), ("min_front_ratio", C.c_double),
                ("min_angle_ratio", C.c_double), ("min_num_valid", C.c_int32)]


class CFundOptions(C.Structure):
    _fields_ = [("max_error", C.c_double), ("confidence", C.c_double), ("min_inlier_ratio", C.c_double),
                ("min_num_trials", C.c_int32), ("max_num_trials", C.c_int32), ("seed", C.c_uint32), ("min_matches", C.c_int32),
                ("min_num_inliers", C.c_int32), ("min_accept_ratio", C.c_double)]


class CMatchOptions(C.Structure):
    _fields_ = [("max_distance", C.c_float), ("max_ratio", C.c_float), ("mutual_best", C.c_int32), ("max_features", C.c_int32)]


class CSiftOptions(C.Structure):
    _fields_ = [("first_octave", C.c_int32), ("num_octaves", C.c_int32), ("peak_threshold", C.c_float), ("edge_threshold", C.c_float),
                ("max_num_features", C.c_int32), ("max_image_size", C.c_int32)]


class CSiftDescOptions(C.Structure):
    _fields_ = [("upright", C.c_int32)]


class CTriOptions(C.Structure):
    _fields_ = [("min_tri_angle_rad", C.c_double), ("max_error_rad", C.c_double), ("confidence", C.c_double),
                ("min_inlier_ratio", C.c_double), ("max_num_trials", C.c_int32), ("exhaustive_threshold", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_uint64, C.c_int)


class COptions(C.Structure):
    _fields_ = [
        ("max_iterations", C.c_int32), ("function_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double), ("initial_radius", C.c_double), ("huber_a", C.c_double),
        ("linear_solver", C.c_int32), ("pcg_tolerance", C.c_double), ("pcg_max_iterations", C.c_int32),
        ("profile", C.c_int32), ("verbose", C.c_int32),
    ]


class CSummary(C.Structure):
    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("num_residuals", C.c_int32), ("num_effective_params", C.c_int32),
        ("n_successful", C.c_int32), ("n_unsuccessful", C.c_int32),
        ("termination", C.c_int32), ("termination_reason", C.c_int32),
        ("pcg_iterations", C.c_int32), ("lm_steps_attempted", C.c_int32),
        ("total_time_s", C.c_double), ("dom_kernel_ms", C.c_double),
        ("dom_kernel_launches", C.c_int32), ("dom_kernel_id", C.c_int32),
        ("linear_solver_used", C.c_int32), ("reserved", C.c_int32),
    ]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


class CExpandOptions(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("patch_cols", "patch_rows", "min_patch_obs", "min_visible", "max_shared_matches", "min_covisible_patches",
                                         "similarity_rank_max", "mayreg_rank_lo", "mayreg_rank_mid", "mayreg_rank_hi", "mayreg_count_mid", "mayreg_count_sum")]


class CMergeOptions(C.Structure):
    _fields_ = [("max_reproj_error", C.c_double), ("mode", C.c_int32), ("frame", C.c_int32)]


class CTrifOptions(C.Structure):
    _fields_ = [("extend_angle_rad", C.c_double), ("tri", CTriOptions)]


# every symbol include/xrsfm_ba.h declares
EXPORTS = [
    "xrsfm_ba_default_options", "xrsfm_ba_version", "xrsfm_ba_create", "xrsfm_ba_comm_unique_id",
    "xrsfm_ba_comm_init", "xrsfm_ba_run", "xrsfm_ba_reset", "xrsfm_ba_download", "xrsfm_ba_destroy",
    "xrsfm_ba_solve", "xrsfm_ba_filter_tracks", "xrsfm_ba_profile_entry", "xrsfm_ba_debug_linearize", "xrsfm_ba_debug_schur_product",
    "xrsfm_ba_debug_cholesky_solve", "xrsfm_ba_debug_set_block_pattern", "xrsfm_ba_debug_pack", "xrsfm_ba_debug_chol_plan", "xrsfm_ba_refine_pose", "xrsfm_ba_refine_pose_options", "xrsfm_ba_debug_comm_hook", "xrsfm_pg_default_options", "xrsfm_pg_solve", "xrsfm_ba_debug_pack_gram", "xrsfm_ba_debug_gram_schedule",
    "xrsfm_tag_default_options", "xrsfm_tag_refine", "xrsfm_ba_refine_poses", "xrsfm_ba_quiesce", "xrsfm_ba_debug_backsub", "xrsfm_ba_device_memory", "xrsfm_ba_download_intrinsics", "xrsfm_ba_debug_wide",
    "xrsfm_ba_debug_device_pack_check", "xrsfm_ba_warmup", "xrsfm_ba_debug_stored_j", "xrsfm_ba_debug_sgroup",
    "xrsfm_ba_debug_reduced_system", "xrsfm_ba_covariance", "xrsfm_ba_point_covariance", "xrsfm_ba_joint_covariance",
    "xrsfm_ba_map_covariance", "xrsfm_ba_debug_backsub_layout", "xrsfm_ba_run_batch", "xrsfm_ba_solve_batch",
    "xrsfm_ba_triangulate_options", "xrsfm_ba_triangulate_tracks", "xrsfm_ba_debug_lin_scalars", "xrsfm_ba_debug_resident_rows",
    "xrsfm_ba_absolute_pose_options", "xrsfm_ba_absolute_pose", "xrsfm_ba_debug_pose_samples",
    "xrsfm_ba_two_view_options_default", "xrsfm_ba_two_view_init", "xrsfm_ba_debug_two_view_samples",
    "xrsfm_ba_verify_pairs_options", "xrsfm_ba_verify_pairs", "xrsfm_ba_debug_fund_samples",
    "xrsfm_ba_match_options_default", "xrsfm_ba_match_descriptors", "xrsfm_ba_debug_match_table",
    "xrsfm_ba_debug_cam_stage",
    "xrsfm_ba_sift_options_default", "xrsfm_ba_detect_keypoints", "xrsfm_ba_debug_sift_taps", "xrsfm_ba_debug_sift_levels",
    "xrsfm_ba_debug_sift_offsets",
    "xrsfm_ba_sift_desc_options_default", "xrsfm_ba_extract_features", "xrsfm_ba_debug_sift_gradient", "xrsfm_ba_debug_sift_describe",
    "xrsfm_ba_frames_create", "xrsfm_ba_frames_from_images", "xrsfm_ba_frames_info", "xrsfm_ba_frames_download", "xrsfm_ba_frames_match",
    "xrsfm_ba_frames_destroy",
    "xrsfm_ba_expand_options_default", "xrsfm_ba_expand_candidates", "xrsfm_ba_frames_expand", "xrsfm_ba_debug_expand_tracks",
    "xrsfm_ba_debug_expand_covis",
    "xrsfm_ba_merge_options_default", "xrsfm_ba_merge_tracks", "xrsfm_ba_debug_merge_components",
    "xrsfm_ba_trif_options_default", "xrsfm_ba_triangulate_frames",
]
# declared too, but kept apart: tests/test_capi_cpu.py collects the header's names with a pattern of letters and underscores only
EXPORTS_WITH_DIGITS = ["xrsfm_ba_debug_match_top2"]

# xrsfm_ba_debug_reduced_system / debug_chol_plan: the schedule facts, in order (include/xrsfm_ba.h)
CHOL_FACTS = ("T", "levels", "ordering", "schedule", "macro_levels", "split_levels", "la_depth", "fill_rest", "rest_apart", "packed",
              "bwd", "height_mask", "cw", "blocks", "n", "tiles_nz")
SCHEDULES = ("level", "panel", "lookahead")
BWD_FORMS = ("fused", "per_level", "all", "chunk", "push")


def _facts(v) -> dict:
    f = dict(zip(CHOL_FACTS, (int(x) for x in v)))
    f["schedule"] = SCHEDULES[f["schedule"]]
    f["bwd"] = BWD_FORMS[f["bwd"]]
    f["rest_apart"] = bool(f["rest_apart"]); f["packed"] = bool(f["packed"])
    # pivot-tile heights in rows: a tile column of m cameras has m * cw rows
    f["heights"] = sorted(m * f["cw"] for m in range(1, 31) if (f["height_mask"] >> m) & 1)
    return f

SOLVER_PCG, SOLVER_CHOLESKY, SOLVER_AUTO = 0, 1, 2
SOLVER_RESIDENT = 3     # the whole LM loop in one kernel launch (local-BA-sized problems: include/xrsfm_ba.h)
BATCH_MAX = 4096        # XRSFM_BA_BATCH_MAX: most contexts of one xrsfm_ba_run_batch
TRI_MAX_OBS = 128       # XRSFM_BA_TRI_MAX_OBS: longest track xrsfm_ba_triangulate_tracks attempts
TRI_LOCAL_BIT = 1 << 30  # best_trial: the locally optimised model of that trial is the one returned
POSE_MAX_CORR = 8192    # XRSFM_BA_POSE_MAX_CORR: most correspondences of a frame xrsfm_ba_absolute_pose attempts
POSE_MAX_TRIALS = 16384  # XRSFM_BA_POSE_MAX_TRIALS
POSE_LOCAL_BIT = 1 << 30  # best_trial: the locally optimised (EPnP) model of that trial is the one returned
INIT_MAX_MATCHES = 8192  # XRSFM_BA_INIT_MAX_MATCHES: most matches of a pair xrsfm_ba_two_view_init attempts
INIT_MAX_TRIALS = 64     # XRSFM_BA_INIT_MAX_TRIALS
INIT_SLOT_STRIDE = 16    # best_trial of xrsfm_ba_two_view_init: trial * 16 + model slot
FUND_MAX_MATCHES = 8192  # XRSFM_BA_FUND_MAX_MATCHES: most matches of a pair xrsfm_ba_verify_pairs attempts
FUND_MAX_TRIALS = 16384  # XRSFM_BA_FUND_MAX_TRIALS
FUND_LOCAL_BIT = 1 << 30  # best_trial: the 8-point local model of that trial is the one returned
MATCH_MAX_FEATURES = 16384  # XRSFM_BA_MATCH_MAX_FEATURES: most descriptors of a frame xrsfm_ba_match_descriptors takes
MATCH_DIM = 128          # XRSFM_BA_MATCH_DIM
MATCH_TABLE_SIZE = (1 << 18) + 1  # entries of xrsfm_ba_debug_match_table
SIFT_MAX_TAPS = 33       # XRSFM_BA_SIFT_MAX_TAPS
SIFT_MAX_OCTAVES = 8     # XRSFM_BA_SIFT_MAX_OCTAVES
EINVAL, ESTATE = -1, -5

ERRORS = {-1: "EINVAL", -2: "ENODEV (no HIP device / HIP error; there is no CPU fallback)", -3: "ENOMEM",
          -4: "ECOMM", -5: "ESTATE", -6: "ETOOBIG", -7: "EINTERNAL (unexpected exception inside the library)",
          -8: "ESINGULAR (the undamped reduced camera matrix is not positive definite)"}
ESINGULAR = -8

_lib = None


def load(path: str | None = None):
    """dlopen libxrsfm_ba.so.  torch (if used in this process) must be imported
    first so both share one HIP runtime (same SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    path = path or os.environ.get("XRSFM_BA_LIB") or _build.LIB      # XRSFM_BA_LIB: developer override (ablation builds)
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                           "the BA path has no fallback implementation")
    lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    vp = C.c_void_p
    lib.xrsfm_ba_default_options.argtypes = [C.POINTER(COptions)]; lib.xrsfm_ba_default_options.restype = None
    lib.xrsfm_ba_version.argtypes = [C.POINTER(C.c_int)]; lib.xrsfm_ba_version.restype = C.c_int
    lib.xrsfm_ba_create.argtypes = [C.POINTER(CProblem), C.c_int, C.POINTER(vp)]; lib.xrsfm_ba_create.restype = C.c_int
    lib.xrsfm_ba_comm_unique_id.argtypes = [C.c_char_p]; lib.xrsfm_ba_comm_unique_id.restype = C.c_int
    lib.xrsfm_ba_comm_init.argtypes = [vp, C.c_int, C.c_int, C.c_char_p]; lib.xrsfm_ba_comm_init.restype = C.c_int
    lib.xrsfm_ba_run.argtypes = [vp, C.POINTER(COptions), C.POINTER(CSummary)]; lib.xrsfm_ba_run.restype = C.c_int
    lib.xrsfm_ba_reset.argtypes = [vp]; lib.xrsfm_ba_reset.restype = C.c_int
    lib.xrsfm_ba_download.argtypes = [vp, _c_double_p, _c_double_p, _c_double_p]; lib.xrsfm_ba_download.restype = C.c_int
    lib.xrsfm_ba_destroy.argtypes = [vp]; lib.xrsfm_ba_destroy.restype = None
    lib.xrsfm_ba_solve.argtypes = [C.POINTER(COptions), C.POINTER(CProblem), C.POINTER(CSummary)]; lib.xrsfm_ba_solve.restype = C.c_int
    lib.xrsfm_ba_filter_tracks.argtypes = [C.POINTER(CProblem), C.c_double, C.c_double, _c_uint8_p, _c_uint8_p, _c_double_p,
                                            _c_double_p, _c_int32_p]
    lib.xrsfm_ba_filter_tracks.restype = C.c_int
    lib.xrsfm_ba_debug_linearize.argtypes = [vp, C.c_double, C.c_int] + [_c_double_p] * 8
    lib.xrsfm_ba_debug_linearize.restype = C.c_int
    lib.xrsfm_ba_debug_schur_product.argtypes = [vp, C.c_double, _c_double_p, _c_double_p, _c_double_p]
    lib.xrsfm_ba_debug_schur_product.restype = C.c_int
    lib.xrsfm_ba_debug_cholesky_solve.argtypes = [vp, C.c_double, _c_double_p, _c_double_p]
    lib.xrsfm_ba_debug_cholesky_solve.restype = C.c_int
    if hasattr(lib, "xrsfm_ba_debug_stored_j"):
        lib.xrsfm_ba_debug_stored_j.argtypes = [vp, C.POINTER(C.c_int32)]
        lib.xrsfm_ba_debug_stored_j.restype = C.c_int
    if hasattr(lib, "xrsfm_ba_debug_backsub"):      # (absent in the round-2 repro builds of tools/backsub_waves_probe.py)
        lib.xrsfm_ba_debug_backsub.argtypes = [vp] + [_c_double_p] * 6
        lib.xrsfm_ba_debug_backsub.restype = C.c_int
    if hasattr(lib, "xrsfm_ba_debug_backsub_layout"):
        lib.xrsfm_ba_debug_backsub_layout.argtypes = [vp, _c_int32_p, _c_int32_p, _c_double_p, _c_int32_p] + [_c_double_p] * 3
        lib.xrsfm_ba_debug_backsub_layout.restype = C.c_int
    if hasattr(lib, "xrsfm_ba_debug_cam_stage"):       # (absent in a parent build loaded through XRSFM_BA_LIB for an A/B run)
        lib.xrsfm_ba_debug_cam_stage.argtypes = [vp, _c_int32_p]
        lib.xrsfm_ba_debug_cam_stage.restype = C.c_int
    lib.xrsfm_ba_debug_set_block_pattern.argtypes = [vp, C.c_int, _c_int32_p]
    lib.xrsfm_ba_debug_set_block_pattern.restype = C.c_int
    lib.xrsfm_pg_default_options.argtypes = [C.POINTER(CPgOptions)]
    lib.xrsfm_pg_default_options.restype = None
    lib.xrsfm_ba_refine_poses.argtypes = [C.POINTER(COptions), C.c_int32, _c_int32_p, _c_double_p, _c_int32_p, _c_double_p, _c_double_p,
                                          _c_uint8_p, _c_double_p, _c_double_p, C.POINTER(CSummary)]
    lib.xrsfm_ba_refine_poses.restype = C.c_int
    lib.xrsfm_pg_solve.argtypes = [C.POINTER(CPgOptions), C.POINTER(CPgProblem), C.POINTER(CPgSummary)]
    lib.xrsfm_pg_solve.restype = C.c_int
    lib.xrsfm_tag_default_options.argtypes = [C.POINTER(CPgOptions)]
    lib.xrsfm_tag_default_options.restype = None
    lib.xrsfm_tag_refine.argtypes = [C.POINTER(CPgOptions), C.POINTER(CTagProblem), C.c_int32, C.POINTER(CPgSummary)]
    lib.xrsfm_tag_refine.restype = C.c_int
    lib.xrsfm_ba_debug_comm_hook.argtypes = [C.c_void_p, C.c_int, C.c_int, ALLREDUCE_FN, C.c_void_p]
    lib.xrsfm_ba_debug_comm_hook.restype = C.c_int
    lib.xrsfm_ba_refine_pose_options.argtypes = [C.POINTER(COptions)]
    lib.xrsfm_ba_refine_pose_options.restype = None
    lib.xrsfm_ba_refine_pose.argtypes = [C.POINTER(COptions), C.c_int32, _c_double_p, C.c_int32, _c_double_p, _c_double_p, _c_uint8_p,
                                         _c_double_p, _c_double_p, C.POINTER(CSummary)]
    lib.xrsfm_ba_refine_pose.restype = C.c_int
    lib.xrsfm_ba_debug_pack_gram.argtypes = [C.POINTER(CProblem), _c_int32_p, _c_int32_p, _c_uint8_p, _c_int32_p]
    lib.xrsfm_ba_debug_pack_gram.restype = C.c_int
    lib.xrsfm_ba_debug_sgroup.argtypes = [C.POINTER(CProblem), C.c_int] + [_c_int32_p] * 7
    lib.xrsfm_ba_debug_sgroup.restype = C.c_int
    lib.xrsfm_ba_debug_chol_plan.argtypes = [C.POINTER(CProblem), _c_int32_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_chol_plan.restype = C.c_int
    lib.xrsfm_ba_debug_reduced_system.argtypes = [vp, C.c_double, _c_int32_p, C.POINTER(C.c_int32), _c_int32_p] + [_c_double_p] * 4
    lib.xrsfm_ba_debug_reduced_system.restype = C.c_int
    lib.xrsfm_ba_debug_pack.argtypes = [C.POINTER(CProblem), _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_pack.restype = C.c_int
    lib.xrsfm_ba_profile_entry.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), _c_double_p, C.POINTER(C.c_int)]
    lib.xrsfm_ba_profile_entry.restype = C.c_int
    lib.xrsfm_ba_covariance.argtypes = [vp, C.c_double, C.c_int32, _c_int32_p, _c_double_p]
    lib.xrsfm_ba_covariance.restype = C.c_int
    lib.xrsfm_ba_point_covariance.argtypes = [vp, C.c_double, C.c_int32, _c_int32_p, _c_double_p]
    lib.xrsfm_ba_point_covariance.restype = C.c_int
    lib.xrsfm_ba_joint_covariance.argtypes = [vp, C.c_double, C.c_int32, _c_int32_p, C.c_int32, _c_int32_p, _c_double_p]
    lib.xrsfm_ba_joint_covariance.restype = C.c_int
    lib.xrsfm_ba_map_covariance.argtypes = [vp, C.c_double, _c_double_p, _c_double_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8)]
    lib.xrsfm_ba_map_covariance.restype = C.c_int
    lib.xrsfm_ba_run_batch.argtypes = [C.c_int32, C.POINTER(vp), C.POINTER(COptions), C.POINTER(CSummary), _c_int32_p]
    lib.xrsfm_ba_run_batch.restype = C.c_int
    lib.xrsfm_ba_solve_batch.argtypes = [C.POINTER(COptions), C.c_int32, C.POINTER(CProblem), C.POINTER(CSummary), _c_int32_p]
    lib.xrsfm_ba_solve_batch.restype = C.c_int
    lib.xrsfm_ba_triangulate_options.argtypes = [C.POINTER(CTriOptions)]
    lib.xrsfm_ba_triangulate_options.restype = None
    lib.xrsfm_ba_triangulate_tracks.argtypes = [C.POINTER(CTriOptions), C.c_int32, _c_double_p, _c_double_p, C.c_int32, _c_int32_p, _c_int32_p,
                                                 _c_double_p, _c_double_p, _c_uint8_p, _c_uint8_p, _c_int32_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_triangulate_tracks.restype = C.c_int
    lib.xrsfm_ba_absolute_pose_options.argtypes = [C.POINTER(CPoseOptions)]
    lib.xrsfm_ba_absolute_pose_options.restype = None
    lib.xrsfm_ba_absolute_pose.argtypes = [C.POINTER(CPoseOptions), C.c_int32, _c_int32_p, _c_double_p, _c_double_p, _c_double_p,
                                            C.POINTER(C.c_uint32), _c_double_p, _c_double_p, _c_uint8_p, _c_uint8_p, _c_int32_p, _c_int32_p,
                                            _c_int32_p]
    lib.xrsfm_ba_absolute_pose.restype = C.c_int
    lib.xrsfm_ba_debug_pose_samples.argtypes = [C.c_uint32, C.c_int32, C.c_int32, _c_int32_p]
    lib.xrsfm_ba_debug_pose_samples.restype = C.c_int
    lib.xrsfm_ba_two_view_options_default.argtypes = [C.POINTER(CTwoViewOptions)]
    lib.xrsfm_ba_two_view_options_default.restype = None
    lib.xrsfm_ba_two_view_init.argtypes = [C.POINTER(CTwoViewOptions), C.c_int32, _c_int32_p, _c_double_p, _c_double_p, _c_double_p,
                                            C.POINTER(C.c_uint32), _c_uint8_p, _c_double_p, _c_double_p, _c_double_p, _c_double_p, _c_uint8_p,
                                            _c_uint8_p, _c_int32_p, _c_uint8_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_two_view_init.restype = C.c_int
    lib.xrsfm_ba_debug_two_view_samples.argtypes = [C.c_uint32, C.c_int32, C.c_int32, _c_int32_p]
    lib.xrsfm_ba_debug_two_view_samples.restype = C.c_int
    lib.xrsfm_ba_verify_pairs_options.argtypes = [C.POINTER(CFundOptions)]
    lib.xrsfm_ba_verify_pairs_options.restype = None
    lib.xrsfm_ba_verify_pairs.argtypes = [C.POINTER(CFundOptions), C.c_int32, _c_int32_p, _c_double_p, _c_double_p, _c_double_p,
                                           C.POINTER(C.c_uint32), _c_uint8_p, _c_double_p, _c_uint8_p, _c_int32_p, _c_int32_p, _c_int32_p,
                                           _c_uint8_p]
    lib.xrsfm_ba_verify_pairs.restype = C.c_int
    lib.xrsfm_ba_debug_fund_samples.argtypes = [C.c_uint32, C.c_int32, C.c_int32, _c_int32_p]
    lib.xrsfm_ba_debug_fund_samples.restype = C.c_int
    lib.xrsfm_ba_match_options_default.argtypes = [C.POINTER(CMatchOptions)]
    lib.xrsfm_ba_match_options_default.restype = None
    lib.xrsfm_ba_match_descriptors.argtypes = [C.POINTER(CMatchOptions), C.c_int32, C.POINTER(C.c_int64), _c_uint8_p, C.c_int32, _c_int32_p, _c_int32_p,
                                                C.c_int64, C.POINTER(C.c_int64), _c_int32_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_match_descriptors.restype = C.c_int
    lib.xrsfm_ba_debug_match_table.argtypes = [C.POINTER(C.c_float)]
    lib.xrsfm_ba_debug_match_table.restype = C.c_int
    lib.xrsfm_ba_debug_match_top2.argtypes = [C.c_int32, _c_uint8_p, C.c_int32, _c_uint8_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_match_top2.restype = C.c_int
    _c_float_p, _c_int64_p, _so = C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(CSiftOptions)
    lib.xrsfm_ba_sift_options_default.argtypes = [_so]
    lib.xrsfm_ba_sift_options_default.restype = None
    lib.xrsfm_ba_detect_keypoints.argtypes = [_so, C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_uint8_p, C.c_int64, _c_int64_p, _c_float_p, _c_int32_p,
                                               C.POINTER(C.c_int8), _c_int32_p]
    lib.xrsfm_ba_detect_keypoints.restype = C.c_int
    lib.xrsfm_ba_debug_sift_taps.argtypes = [C.c_float, _c_float_p, _c_int32_p]
    lib.xrsfm_ba_debug_sift_taps.restype = C.c_int
    lib.xrsfm_ba_debug_sift_levels.argtypes = [_so, C.c_int32, C.c_int32, _c_uint8_p, C.c_int32, _c_float_p, _c_float_p]
    lib.xrsfm_ba_debug_sift_levels.restype = C.c_int
    lib.xrsfm_ba_debug_sift_offsets.argtypes = [_so, C.c_int32, C.c_int32, _c_uint8_p, C.c_int64, _c_int64_p, _c_int32_p, _c_float_p]
    lib.xrsfm_ba_debug_sift_offsets.restype = C.c_int
    _sd = C.POINTER(CSiftDescOptions)
    lib.xrsfm_ba_sift_desc_options_default.argtypes = [_sd]
    lib.xrsfm_ba_sift_desc_options_default.restype = None
    lib.xrsfm_ba_extract_features.argtypes = [_so, _sd, C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_uint8_p, C.c_int64, _c_int64_p, _c_float_p, _c_int32_p,
                                               C.POINTER(C.c_int8), _c_uint8_p, _c_float_p, _c_int32_p]
    lib.xrsfm_ba_extract_features.restype = C.c_int
    lib.xrsfm_ba_debug_sift_gradient.argtypes = [_so, C.c_int32, C.c_int32, _c_uint8_p, C.c_int32, _c_float_p]
    lib.xrsfm_ba_debug_sift_gradient.restype = C.c_int
    lib.xrsfm_ba_debug_sift_describe.argtypes = [_so, _sd, C.c_int32, C.c_int32, _c_uint8_p, C.c_int64, _c_int64_p, _c_int32_p, _c_float_p, _c_float_p, _c_float_p]
    lib.xrsfm_ba_debug_sift_describe.restype = C.c_int
    _u32_p, _u64_p, _i8_p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_int8)
    lib.xrsfm_ba_frames_create.argtypes = [C.c_int32, _c_int64_p, _c_float_p, _c_uint8_p, C.POINTER(vp)]
    lib.xrsfm_ba_frames_create.restype = C.c_int
    lib.xrsfm_ba_frames_from_images.argtypes = [_so, _sd, C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_uint8_p, C.POINTER(vp)]
    lib.xrsfm_ba_frames_from_images.restype = C.c_int
    lib.xrsfm_ba_frames_info.argtypes = [vp, _c_int32_p, _c_int64_p, _u64_p]
    lib.xrsfm_ba_frames_info.restype = C.c_int
    lib.xrsfm_ba_frames_download.argtypes = [vp, C.c_int64, _c_float_p, _c_uint8_p, _c_int32_p, _i8_p, _c_int32_p]
    lib.xrsfm_ba_frames_download.restype = C.c_int
    lib.xrsfm_ba_frames_match.argtypes = [vp, C.POINTER(CMatchOptions), C.POINTER(CFundOptions), C.c_int32, _c_int32_p, _c_int32_p, _c_double_p, _u32_p, C.c_int64,
                                          _c_int64_p, _c_int32_p, _c_int32_p, _c_int32_p, _c_uint8_p, _c_double_p, _c_uint8_p, _c_int32_p, _c_int32_p, _c_int32_p,
                                          _c_uint8_p]
    lib.xrsfm_ba_frames_match.restype = C.c_int
    lib.xrsfm_ba_frames_destroy.argtypes = [vp]
    lib.xrsfm_ba_frames_destroy.restype = None
    _eo = C.POINTER(CExpandOptions)
    _expand_tail = [C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_int32_p, _c_int64_p, _c_int32_p, C.c_int32, _c_int32_p, _c_int32_p, C.c_int32, C.c_int32,
                    C.c_int64, _c_int64_p, _c_int32_p, _c_int32_p, _c_uint8_p, _c_uint8_p, _c_uint8_p, _c_uint8_p, _c_int32_p, C.c_int64, _c_int64_p, _c_int32_p, _c_int64_p]
    lib.xrsfm_ba_expand_options_default.argtypes = [_eo]
    lib.xrsfm_ba_expand_options_default.restype = None
    lib.xrsfm_ba_expand_candidates.argtypes = [_eo, C.c_int32, _c_int64_p, _c_float_p, _c_int32_p, _c_int32_p] + _expand_tail
    lib.xrsfm_ba_expand_candidates.restype = C.c_int
    lib.xrsfm_ba_frames_expand.argtypes = [vp, _eo, _c_int32_p, _c_int32_p] + _expand_tail
    lib.xrsfm_ba_frames_expand.restype = C.c_int
    lib.xrsfm_ba_debug_expand_tracks.argtypes = [C.c_int32, _c_int64_p, C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_int32_p, _c_int32_p, C.c_int64, _c_int64_p,
                                                 _c_int64_p, _c_uint8_p, C.c_int64, _c_int64_p, _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_expand_tracks.restype = C.c_int
    lib.xrsfm_ba_debug_expand_covis.argtypes = [_eo, C.c_int32, _c_int64_p, _c_float_p, _c_int32_p, _c_int32_p, C.c_int32, _c_int32_p, _c_int32_p, _c_int64_p, _c_int32_p,
                                                C.c_int32, C.c_int32, C.c_int64, _c_int64_p, _c_int32_p]
    lib.xrsfm_ba_debug_expand_covis.restype = C.c_int
    _mo = C.POINTER(CMergeOptions)
    _merge_head = [_mo, C.c_int32, _c_int64_p, _c_double_p, _c_uint8_p, _c_double_p, _c_double_p, _c_int32_p, C.c_int32, _c_int32_p, _c_double_p, _c_int64_p, _c_int32_p,
                   C.c_int32, _c_double_p, _c_uint8_p, _c_int32_p]
    lib.xrsfm_ba_merge_options_default.argtypes = [_mo]
    lib.xrsfm_ba_merge_options_default.restype = None
    lib.xrsfm_ba_merge_tracks.argtypes = _merge_head + [_c_uint8_p, _c_int32_p, _c_int32_p, _c_int32_p, _c_int64_p]
    lib.xrsfm_ba_merge_tracks.restype = C.c_int
    lib.xrsfm_ba_debug_merge_components.argtypes = _merge_head + [_c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_merge_components.restype = C.c_int
    lib.xrsfm_ba_trif_options_default.argtypes = [C.POINTER(CTrifOptions)]
    lib.xrsfm_ba_trif_options_default.restype = None
    lib.xrsfm_ba_triangulate_frames.argtypes = [C.POINTER(CTrifOptions), C.c_int32, _c_int64_p, _c_double_p, _c_uint8_p, _c_double_p, _c_double_p, _c_int64_p, _c_int32_p,
                                                C.c_int32, _c_int32_p, C.c_int32, C.c_int32, _c_double_p, _c_uint8_p, _c_int32_p, _c_int32_p, _c_uint8_p, _c_int32_p,
                                                _c_int32_p, _c_int32_p, _c_int32_p, _c_int32_p, _c_int32_p, _c_int64_p]
    lib.xrsfm_ba_triangulate_frames.restype = C.c_int
    _lib = lib
    return lib


def check(code: int, what: str):
    if code != 0:
        raise RuntimeError(f"{what} failed: {code} {ERRORS.get(code, '')}")


def _dp(a):
    return a.ctypes.data_as(_c_double_p) if a is not None else None


def device_count() -> int:
    n = C.c_int(0)
    load().xrsfm_ba_version(C.byref(n))
    return n.value


def quiesce() -> int:
    """xrsfm_ba_quiesce: wait for deferred context releases, free the cached device blocks; returns the bytes that were cached."""
    n = C.c_uint64(0)
    lib = load()
    lib.xrsfm_ba_quiesce.argtypes = [C.POINTER(C.c_uint64)]
    lib.xrsfm_ba_quiesce.restype = C.c_int
    check(lib.xrsfm_ba_quiesce(C.byref(n)), "xrsfm_ba_quiesce")
    return int(n.value)


def default_options(**kw) -> COptions:
    o = COptions()
    load().xrsfm_ba_default_options(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


class ProblemArrays:
    """Owns contiguous numpy arrays of one BA call and the matching C struct."""
    FIELDS = ("cam_q", "cam_t", "cam_const", "cam_intr", "intr_model", "intr_params",
              "points", "point_const", "obs_cam", "obs_pt", "obs_uv")

    def __init__(self, **arr):
        f64 = lambda a, s: np.ascontiguousarray(np.asarray(a, np.float64).reshape(s))
        self.cam_q = f64(arr["cam_q"], (-1, 4)); self.cam_t = f64(arr["cam_t"], (-1, 3))
        n_c = self.cam_q.shape[0]
        cc = arr.get("cam_const")
        self.cam_const = np.ascontiguousarray(np.zeros(n_c, np.uint8) if cc is None else np.asarray(cc, np.uint8))
        self.cam_intr = np.ascontiguousarray(np.asarray(arr["cam_intr"], np.int32))
        self.intr_model = np.ascontiguousarray(np.asarray(arr["intr_model"], np.int32))
        self.intr_params = f64(arr["intr_params"], (-1, 8))
        self.points = f64(arr["points"], (-1, 3))
        pc = arr.get("point_const")
        self.point_const = np.ascontiguousarray(np.zeros(self.points.shape[0], np.uint8) if pc is None else np.asarray(pc, np.uint8))
        self.obs_cam = np.ascontiguousarray(np.asarray(arr["obs_cam"], np.int32))
        self.obs_pt = np.ascontiguousarray(np.asarray(arr["obs_pt"], np.int32))
        self.obs_uv = f64(arr["obs_uv"], (-1, 2))
        if not (self.cam_t.shape[0] == n_c and self.cam_intr.shape[0] == n_c and self.cam_const.shape[0] == n_c):
            raise ValueError("cam_q / cam_t / cam_intr / cam_const disagree on the number of cameras")
        if not (self.obs_pt.shape[0] == self.obs_cam.shape[0] == self.obs_uv.shape[0]):
            raise ValueError("obs_cam / obs_pt / obs_uv disagree on the number of observations")
        if self.point_const.shape[0] != self.points.shape[0] or self.intr_model.shape[0] != self.intr_params.shape[0]:
            raise ValueError("point_const / points or intr_model / intr_params disagree in length")

    @property
    def n_cams(self): return self.cam_q.shape[0]
    @property
    def n_points(self): return self.points.shape[0]
    @property
    def n_obs(self): return self.obs_cam.shape[0]

    def as_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def c_struct(self) -> CProblem:
        i32 = lambda a: a.ctypes.data_as(_c_int32_p)
        u8 = lambda a: a.ctypes.data_as(_c_uint8_p)
        return CProblem(self.n_cams, self.n_points, self.n_obs, self.intr_model.shape[0],
                        _dp(self.cam_q), _dp(self.cam_t), u8(self.cam_const), i32(self.cam_intr),
                        i32(self.intr_model), _dp(self.intr_params), _dp(self.points), u8(self.point_const),
                        i32(self.obs_cam), i32(self.obs_pt), _dp(self.obs_uv))


class Context:
    """Device-resident BA problem (xrsfm_ba_create ... xrsfm_ba_destroy)."""

    def __init__(self, problem: ProblemArrays, device: int = 0):
        self.lib = load()
        self.problem = problem
        self._h = C.c_void_p()
        cs = problem.c_struct()
        check(self.lib.xrsfm_ba_create(C.byref(cs), device, C.byref(self._h)), "xrsfm_ba_create")

    def close(self):
        if self._h:
            self.lib.xrsfm_ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_init(self, n_ranks: int, rank: int, unique_id: bytes):
        check(self.lib.xrsfm_ba_comm_init(self._h, n_ranks, rank, unique_id), "xrsfm_ba_comm_init")

    def comm_hook(self, n_ranks: int, rank: int, allreduce):
        """TEST transport: `allreduce(array, op)` reduces a host float64 array in place across the ranks (op 0 sum, 1 max)."""
        def _cb(user, buf, n, op):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(int(n),)), int(op))
                return 0
            except Exception:      # noqa: BLE001  (must not unwind through the C frame)
                return 1
        self._hook = ALLREDUCE_FN(_cb)       # keep the trampoline alive as long as the context
        check(self.lib.xrsfm_ba_debug_comm_hook(self._h, n_ranks, rank, self._hook, None), "xrsfm_ba_debug_comm_hook")

    def run(self, options: COptions | None = None) -> CSummary:
        options = options or default_options()
        s = CSummary()
        check(self.lib.xrsfm_ba_run(self._h, C.byref(options), C.byref(s)), "xrsfm_ba_run")
        return s

    def reset(self):
        check(self.lib.xrsfm_ba_reset(self._h), "xrsfm_ba_reset")

    def download(self, out=None):
        """out: optional (cam_q, cam_t, points) arrays to write into (the C++ adapter writes into the map's own storage; fresh
        numpy arrays of tens of MB cost their first-touch page faults on top of the copy)."""
        p = self.problem
        if out is None:
            q = np.empty_like(p.cam_q); t = np.empty_like(p.cam_t); P = p.points.copy()
        else:
            q, t, P = out
            # (not `assert`: stripped under python -O, and the C function writes through these pointers unchecked)
            if not (q.shape == p.cam_q.shape and t.shape == p.cam_t.shape and P.shape == p.points.shape):
                raise ValueError("download(out=...): shapes must equal the problem's cam_q / cam_t / points")
            if not all(a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable for a in (q, t, P)):
                raise ValueError("download(out=...): arrays must be writable C-contiguous float64")
            if P is not p.points:
                P[...] = p.points      # points that take no part in the problem keep their input value
        check(self.lib.xrsfm_ba_download(self._h, _dp(q), _dp(t), _dp(P)), "xrsfm_ba_download")
        return q, t, P

    def covariance(self, cams, huber_a: float = 5.99) -> np.ndarray:
        """Marginal covariance [n][6][6] (tangent space: rotation 3, translation 3) of the cameras `cams` at the current device
        state: xrsfm_ba_covariance.  Raises RuntimeError naming the code (EINVAL, ETOOBIG, ESINGULAR) on failure."""
        sel = np.ascontiguousarray(cams, np.int32).reshape(-1)
        cov = np.zeros((sel.shape[0], 6, 6))
        check(self.lib.xrsfm_ba_covariance(self._h, huber_a, sel.shape[0], sel.ctypes.data_as(_c_int32_p), _dp(cov)), "xrsfm_ba_covariance")
        return cov

    def point_covariance(self, points, huber_a: float = 5.99) -> np.ndarray:
        """Marginal covariance [n][3][3] of the 3-D points `points` (the caller's indices) at the current device state:
        xrsfm_ba_point_covariance.  Raises RuntimeError naming the code (EINVAL, ETOOBIG, ESINGULAR) on failure."""
        sel = np.ascontiguousarray(points, np.int32).reshape(-1)
        cov = np.zeros((sel.shape[0], 3, 3))
        check(self.lib.xrsfm_ba_point_covariance(self._h, huber_a, sel.shape[0], sel.ctypes.data_as(_c_int32_p), _dp(cov)), "xrsfm_ba_point_covariance")
        return cov

    def joint_covariance(self, cams, points, huber_a: float = 5.99) -> np.ndarray:
        """Joint covariance [N][N], N = 6 len(cams) + 3 len(points), of the cameras `cams` (first, 6 tangent rows each) and the 3-D
        points `points` (the caller's indices) with every cross block, at the current device state: xrsfm_ba_joint_covariance.
        Raises RuntimeError naming the code (EINVAL, ETOOBIG, ESINGULAR, ENOMEM) on failure."""
        cs = np.ascontiguousarray(cams, np.int32).reshape(-1)
        ps = np.ascontiguousarray(points, np.int32).reshape(-1)
        n = 6 * cs.shape[0] + 3 * ps.shape[0]
        cov = np.zeros((n, n))
        check(self.lib.xrsfm_ba_joint_covariance(self._h, huber_a, cs.shape[0], cs.ctypes.data_as(_c_int32_p), ps.shape[0], ps.ctypes.data_as(_c_int32_p), _dp(cov)),
              "xrsfm_ba_joint_covariance")
        return cov

    def map_covariance(self, cameras: bool = True, points: bool = True, huber_a: float = 5.99) -> dict:
        """Marginal covariance of EVERY camera ([n_cams][6][6]) and EVERY point ([n_points][3][3], the caller's indices) at the current
        device state by selected inversion of the tile factor: xrsfm_ba_map_covariance.  Returns a dict with "cam_cov" / "cam_status"
        (cameras=True) and "pt_cov" / "pt_status" (points=True); status 0 estimated, 1 all constant, 2 not in the program (zero
        blocks).  Raises RuntimeError naming the code (EINVAL, ETOOBIG, ESINGULAR, ENOMEM) on failure."""
        p = self.problem
        out = {}
        if cameras:
            out["cam_cov"] = np.zeros((p.n_cams, 6, 6)); out["cam_status"] = np.zeros(p.n_cams, np.uint8)
        if points:
            out["pt_cov"] = np.zeros((p.n_points, 3, 3)); out["pt_status"] = np.zeros(p.n_points, np.uint8)
        u8 = lambda k: out[k].ctypes.data_as(C.POINTER(C.c_uint8)) if k in out else None
        check(self.lib.xrsfm_ba_map_covariance(self._h, huber_a, _dp(out["cam_cov"]) if cameras else None, _dp(out["pt_cov"]) if points else None,
                                               u8("cam_status"), u8("pt_status")), "xrsfm_ba_map_covariance")
        return out

    def debug_linearize(self, huber_a: float = 5.99, use_scaling: bool = False):
        p = self.problem
        out = dict(r=np.zeros((p.n_obs, 2)), Jc=np.zeros((p.n_obs, 2, 6)), Jp=np.zeros((p.n_obs, 2, 3)),
                   Hpp=np.zeros((p.n_points, 6)), gp=np.zeros((p.n_points, 3)),
                   Hcc_diag=np.zeros((p.n_cams, 6)), gc=np.zeros((p.n_cams, 6)))
        cost = C.c_double(0)
        check(self.lib.xrsfm_ba_debug_linearize(self._h, huber_a, int(use_scaling), _dp(out["r"]), _dp(out["Jc"]),
                                                _dp(out["Jp"]), _dp(out["Hpp"]), _dp(out["gp"]), _dp(out["Hcc_diag"]),
                                                _dp(out["gc"]), C.cast(C.byref(cost), _c_double_p)), "debug_linearize")
        out["cost"] = cost.value
        return out

    def debug_schur_product(self, radius: float, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float64)
        y = np.zeros_like(x); b = np.zeros_like(x)
        check(self.lib.xrsfm_ba_debug_schur_product(self._h, radius, _dp(x), _dp(y), _dp(b)), "debug_schur_product")
        return y, b


    def debug_stored_j(self) -> bool:
        """True while the context keeps the per-observation residual / Jacobian stored (False: J-free linearisation)."""
        v = C.c_int32(0)
        check(self.lib.xrsfm_ba_debug_stored_j(self._h, C.byref(v)), "debug_stored_j")
        return bool(v.value)

    def debug_lin_scalars(self) -> dict:
        """After debug_linearize / debug_wide: the scalars of the current linearisation as a run reads them (gradient_max)."""
        out = np.zeros(4)
        self.lib.xrsfm_ba_debug_lin_scalars.argtypes = [C.c_void_p, _c_double_p]
        self.lib.xrsfm_ba_debug_lin_scalars.restype = C.c_int
        check(self.lib.xrsfm_ba_debug_lin_scalars(self._h, _dp(out)), "xrsfm_ba_debug_lin_scalars")
        return dict(sum_rho=float(out[0]), xnorm2_pts=float(out[1]), gradmax_pts=float(out[2]), gradmax_cams=float(out[3]))

    ROW_FIELDS = ("cost", "change", "gmax", "step", "rho", "radius", "it")

    def debug_resident_rows(self, options: COptions | None = None):
        """run() with SOLVER_RESIDENT plus the iteration rows of that launch: (summary, rows), rows a list of dicts over ROW_FIELDS
        (one per evaluated point and per rejected step; xrsfm_ba_debug_resident_rows)."""
        options = options or default_options()
        s = CSummary()
        buf = np.zeros((int(options.max_iterations) + 1, 7))
        n = C.c_int32(0)
        self.lib.xrsfm_ba_debug_resident_rows.argtypes = [C.c_void_p, C.POINTER(COptions), C.POINTER(CSummary), _c_double_p, C.POINTER(C.c_int32)]
        self.lib.xrsfm_ba_debug_resident_rows.restype = C.c_int
        check(self.lib.xrsfm_ba_debug_resident_rows(self._h, C.byref(options), C.byref(s), _dp(buf), C.byref(n)), "xrsfm_ba_debug_resident_rows")
        rows = [dict(zip(self.ROW_FIELDS, (float(v) for v in buf[i]))) for i in range(int(n.value))]
        for r in rows:
            r["it"] = int(r["it"])
        return s, rows

    def debug_cholesky_solve(self, radius: float, want_S: bool = False):
        n = 6 * self.problem.n_cams
        y = np.zeros((self.problem.n_cams, 6))
        S = np.zeros((n, n)) if want_S else None
        check(self.lib.xrsfm_ba_debug_cholesky_solve(self._h, radius, _dp(y), _dp(S)), "debug_cholesky_solve")
        return y, S

    def debug_reduced_system(self, radius: float, want_y: bool = True) -> dict:
        """After debug_linearize (bal9: debug_wide): the damped reduced system as the tile factorisation reads it — S as a symmetric
        scipy.sparse CSR matrix in camera order (cw unknowns per camera), b [n_cams][cw] — the solution y of the same
        factorisation (want_y) and the schedule facts (CHOL_FACTS)."""
        import scipy.sparse as sp
        lib = self.lib
        facts = np.zeros(16, np.int32)
        nb = C.c_int32(0)
        check(lib.xrsfm_ba_debug_reduced_system(self._h, radius, facts.ctypes.data_as(_c_int32_p), C.byref(nb), None, None, None, None, None),
              "xrsfm_ba_debug_reduced_system")
        f = _facts(facts)
        nc, cw, m = self.problem.n_cams, f["cw"], nb.value
        rc = np.zeros((max(m, 1), 2), np.int32); blk = np.zeros((max(m, 1), cw, cw)); diag = np.zeros((nc, cw, cw)); b = np.zeros((nc, cw))
        y = np.zeros((nc, cw)) if want_y else None
        check(lib.xrsfm_ba_debug_reduced_system(self._h, radius, facts.ctypes.data_as(_c_int32_p), C.byref(nb), rc.ctypes.data_as(_c_int32_p),
                                                _dp(blk), _dp(diag), _dp(b), _dp(y)), "xrsfm_ba_debug_reduced_system")
        rc, blk = rc[:m], blk[:m]
        ar = np.arange(cw)
        def coo(rows, cols, vals):      # [k] block rows / columns, [k][cw][cw] values -> scalar COO triplets
            shape = (len(rows), cw, cw)
            r = np.broadcast_to(cw * rows[:, None, None] + ar[None, :, None], shape)
            c = np.broadcast_to(cw * cols[:, None, None] + ar[None, None, :], shape)
            return r.ravel(), c.ravel(), vals.ravel()
        cams = np.arange(nc)
        parts = [coo(cams, cams, diag), coo(rc[:, 0], rc[:, 1], blk), coo(rc[:, 1], rc[:, 0], blk.transpose(0, 2, 1))]
        r, c, v = (np.concatenate(x) for x in zip(*parts))
        S = sp.csr_matrix((v, (r, c)), shape=(nc * cw, nc * cw))
        return dict(S=S, b=b, y=y, facts=f, blk_rc=rc)

    def download_intrinsics(self) -> np.ndarray:
        """bal9 mode: intr_params with the refined {f, k1, k2} of the cameras that keep their intrinsics variable."""
        out = np.array(self.problem.intr_params, copy=True)
        self.lib.xrsfm_ba_download_intrinsics.argtypes = [C.c_void_p, _c_double_p]
        self.lib.xrsfm_ba_download_intrinsics.restype = C.c_int
        check(self.lib.xrsfm_ba_download_intrinsics(self._h, _dp(out)), "xrsfm_ba_download_intrinsics")
        return out

    def debug_wide(self, huber_a: float = 5.99, radius: float | None = None) -> dict:
        """bal9 contexts: scaled linearisation (and, with a radius, the reduced-system step) in caller order."""
        p = self.problem
        out = dict(r=np.zeros((p.n_obs, 2)), Jc=np.zeros((p.n_obs, 2, 9)), Jp=np.zeros((p.n_obs, 2, 3)), Hcc_diag=np.zeros((p.n_cams, 9)),
                   gc=np.zeros((p.n_cams, 9)))
        y = np.zeros((p.n_cams, 9)) if radius is not None else None
        cost = C.c_double(0)
        self.lib.xrsfm_ba_debug_wide.argtypes = [C.c_void_p, C.c_double, C.c_double, C.POINTER(C.c_double)] + [_c_double_p] * 6
        self.lib.xrsfm_ba_debug_wide.restype = C.c_int
        check(self.lib.xrsfm_ba_debug_wide(self._h, huber_a, float(radius or 1.0), C.byref(cost), _dp(out["r"]), _dp(out["Jc"]), _dp(out["Jp"]),
                                          _dp(out["Hcc_diag"]), _dp(out["gc"]), _dp(y)), "xrsfm_ba_debug_wide")
        out["cost"] = cost.value
        if y is not None:
            out["y"] = y
        return out

    def debug_backsub(self) -> dict:
        """After debug_cholesky_solve: one k_backsub launch; per-item partials and the candidate state in PACKED order."""
        st = debug_pack(self.problem)
        ni, npk, nc = st["items"], st["active_points"], self.problem.n_cams
        out = dict(part_model=np.zeros(ni), part_step2=np.zeros(ni), cand_points=np.zeros((npk, 3)), point_step=np.zeros((npk, 3)),
                   cand_cam_q=np.zeros((nc, 4)), cand_cam_t=np.zeros((nc, 3)))
        check(self.lib.xrsfm_ba_debug_backsub(self._h, *[_dp(out[k]) for k in ("part_model", "part_step2", "cand_points", "point_step",
                                                                                  "cand_cam_q", "cand_cam_t")]), "debug_backsub")
        return out

    def debug_cam_stage(self) -> tuple:
        """xrsfm_ba_debug_cam_stage: (tiles on the staged route of k_backsub, tiles on the gather route)."""
        counts = np.zeros(2, np.int32)
        check(self.lib.xrsfm_ba_debug_cam_stage(self._h, counts.ctypes.data_as(_c_int32_p)), "debug_cam_stage")
        return int(counts[0]), int(counts[1])

    def debug_backsub_layout(self, after_backsub: bool = False, scales: bool = False) -> dict:
        """xrsfm_ba_debug_backsub_layout: pt_orig [n_points_packed], item_tiles [n_items][2] (first tile, tiles), the flags step_prep
        (the last step ran k_backsub<true>) and stored_j.  after_backsub (needs a debug_backsub on the current step): also campart
        [2][n_cams] and cand_intr [n_cams][3].  scales (needs a linearisation only): also the Jacobi scales scale_c [n_cams][6 or 9]
        and scale_p [n_points_packed][3] — bal9 contexts have no unscaled linearisation to recompute them from (debug_wide returns
        the scaled one), and a test of the candidate state needs the scales the kernel used."""
        st = debug_pack(self.problem)
        nc = self.problem.n_cams
        out = dict(pt_orig=np.zeros(st["active_points"], np.int32), item_tiles=np.zeros((st["items"], 2), np.int32))
        flags = np.zeros(2, np.int32)
        if after_backsub:
            out["campart"] = np.zeros((2, nc)); out["cand_intr"] = np.zeros((nc, 3))
        if scales:
            cw = 9 if (self.problem.cam_const & 4).any() else 6
            out["scale_c"] = np.zeros((nc, cw)); out["scale_p"] = np.zeros((st["active_points"], 3))
        i32 = lambda a: a.ctypes.data_as(_c_int32_p)
        check(self.lib.xrsfm_ba_debug_backsub_layout(self._h, i32(out["pt_orig"]), i32(out["item_tiles"]), _dp(out.get("campart")), i32(flags),
                                                     _dp(out.get("cand_intr")), _dp(out.get("scale_c")), _dp(out.get("scale_p"))),
              "debug_backsub_layout")
        out["step_prep"] = bool(flags[0]); out["stored_j"] = bool(flags[1])
        out["slot_obs"] = st["slot_obs"]
        return out

    def debug_backsub_caller_order(self) -> dict:
        """debug_backsub with everything in the CALLER's order: cand_points / point_step [n_points][3] (rows of points without an
        observation: the input point / zero) and `packed` [n_points] (False for those rows); per work item part_model / part_step2
        [n_items], item_obs (list of the caller's observation indices of the item) and item_points (list of the caller's point
        indices headed in the item); cand_cam_q / cand_cam_t / cand_intr per camera, campart [2][n_cams]; the Jacobi scales scale_c, scale_p [n_points][3]
        (1 for points without an observation); step_prep, stored_j."""
        raw = self.debug_backsub()
        lay = self.debug_backsub_layout(after_backsub=True, scales=True)
        p = self.problem
        po = lay["pt_orig"]
        out = {k: raw[k] for k in ("part_model", "part_step2", "cand_cam_q", "cand_cam_t")}
        out.update({k: lay[k] for k in ("campart", "cand_intr", "step_prep", "stored_j", "item_tiles", "scale_c")})
        out["scale_p"] = np.ones((p.n_points, 3)); out["scale_p"][po] = lay["scale_p"]
        out["cand_points"] = np.array(p.points, copy=True); out["cand_points"][po] = raw["cand_points"]
        out["point_step"] = np.zeros((p.n_points, 3)); out["point_step"][po] = raw["point_step"]
        out["packed"] = np.zeros(p.n_points, bool); out["packed"][po] = True
        so = lay["slot_obs"]
        out["item_obs"], out["item_points"] = [], []
        for first, n in lay["item_tiles"]:
            o = so[64 * first:64 * (first + n)]
            o = o[o >= 0]
            out["item_obs"].append(o)
            out["item_points"].append(np.unique(p.obs_pt[o]))
        return out

    def debug_set_block_pattern(self, row_col: np.ndarray):
        rc = np.ascontiguousarray(row_col, np.int32).reshape(-1, 2)
        check(self.lib.xrsfm_ba_debug_set_block_pattern(self._h, rc.shape[0], rc.ctypes.data_as(_c_int32_p)), "debug_set_block_pattern")

    def profile(self) -> dict:
        """Per-kernel HIP-event totals of the last run with options.profile != 0: name -> (ms, launches)."""
        out = {}
        i = 0
        while True:
            name = C.c_char_p(); ms = C.c_double(0); n = C.c_int(0)
            if self.lib.xrsfm_ba_profile_entry(self._h, i, C.byref(name), C.cast(C.byref(ms), _c_double_p), C.byref(n)) != 0:
                break
            out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(load().xrsfm_ba_comm_unique_id(buf), "xrsfm_ba_comm_unique_id")
    return buf.raw


def solve(problem: ProblemArrays, options: COptions | None = None) -> CSummary:
    """One-shot xrsfm_ba_solve: results are written into problem.cam_q / cam_t / points."""
    options = options or default_options()
    s = CSummary()
    cs = problem.c_struct()
    check(load().xrsfm_ba_solve(C.byref(options), C.byref(cs), C.byref(s)), "xrsfm_ba_solve")
    return s


def run_batch(contexts, options: COptions, n_ctx: int | None = None):
    """xrsfm_ba_run_batch: every Context of `contexts` solved by XRSFM_BA_SOLVER_RESIDENT in ONE launch (options.linear_solver must
    be SOLVER_RESIDENT).  Returns (code, [summary per context], codes): the call does not raise, because with code EINVAL the batch
    may be partly advanced and `codes` (int32 per context: 0 or EINVAL) says where.  An entry may be None (a NULL pointer), and
    n_ctx overrides the count handed to the library (both for the argument checks; the array holds max(n_ctx, len) entries, the
    tail repeating the last one)."""
    lib = load()
    hs = [None if c is None else c._h for c in contexts]
    n = len(hs) if n_ctx is None else int(n_ctx)
    m = max(n, len(hs), 1)
    arr = (C.c_void_p * m)(*(hs + [hs[-1] if hs else None] * (m - len(hs))))
    sums = (CSummary * m)()
    codes = np.zeros(m, np.int32)
    code = lib.xrsfm_ba_run_batch(n, arr, C.byref(options), sums, codes.ctypes.data_as(_c_int32_p))
    k = max(min(n, m), 0)
    return code, [sums[i] for i in range(k)], codes[:k]


def solve_batch(problems, options: COptions):
    """One-shot xrsfm_ba_solve_batch: results are written into every problem's cam_q / cam_t / points; a problem whose code is
    non-zero keeps its arrays.  Returns (code, [summary per problem], codes) like run_batch."""
    lib = load()
    n = len(problems)
    cs = (CProblem * max(n, 1))(*[p.c_struct() for p in problems])
    sums = (CSummary * max(n, 1))()
    codes = np.zeros(max(n, 1), np.int32)
    code = lib.xrsfm_ba_solve_batch(C.byref(options), n, cs, sums, codes.ctypes.data_as(_c_int32_p))
    return code, [sums[i] for i in range(n)], codes[:n]


def filter_tracks(problem: ProblemArrays, max_reproj_error: float, min_tri_angle_rad: float) -> dict:
    """xrsfm_ba_filter_tracks: masks and per-track statistics of the reference's FilterPoints3d."""
    obs_del = np.zeros(problem.n_obs, np.uint8); out = np.zeros(problem.n_points, np.uint8)
    err = np.zeros(problem.n_points); ang = np.zeros(problem.n_points); cnt = np.zeros(2, np.int32)
    cs = problem.c_struct()
    check(load().xrsfm_ba_filter_tracks(C.byref(cs), max_reproj_error, min_tri_angle_rad, obs_del.ctypes.data_as(_c_uint8_p),
                                        out.ctypes.data_as(_c_uint8_p), _dp(err), _dp(ang), cnt.ctypes.data_as(_c_int32_p)),
          "xrsfm_ba_filter_tracks")
    return dict(obs_delete=obs_del, track_outlier=out, track_error=err, track_angle=ang, num_filtered=cnt)


def triangulate_options(**overrides) -> CTriOptions:
    """xrsfm_ba_triangulate_options: the settings of the reference's CreatePoint3d1."""
    o = CTriOptions()
    load().xrsfm_ba_triangulate_options(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def triangulate_tracks(cam_q, cam_t, trk_ptr, obs_cam, obs_xy, options: CTriOptions | None = None) -> dict:
    """xrsfm_ba_triangulate_tracks: one robust triangulation per track (observations trk_ptr[j] .. trk_ptr[j+1], normalised image
    coordinates, Tcw poses).  points of tracks whose status is not 1 stay 0 here (the C call leaves them untouched)."""
    o = options if options is not None else triangulate_options()
    cam_q = np.ascontiguousarray(cam_q, np.float64).reshape(-1, 4); cam_t = np.ascontiguousarray(cam_t, np.float64).reshape(-1, 3)
    trk_ptr = np.ascontiguousarray(trk_ptr, np.int32); obs_cam = np.ascontiguousarray(obs_cam, np.int32)
    obs_xy = np.ascontiguousarray(obs_xy, np.float64).reshape(-1, 2)
    if len(cam_q) != len(cam_t) or trk_ptr.ndim != 1 or len(trk_ptr) < 1 or len(obs_cam) != len(obs_xy):
        raise ValueError("triangulate_tracks: inconsistent array shapes")
    nt, no = len(trk_ptr) - 1, len(obs_cam)
    if nt > 0 and trk_ptr[-1] != no:
        raise ValueError("triangulate_tracks: trk_ptr[-1] must be the number of observations")
    points = np.zeros((nt, 3)); status = np.zeros(nt, np.uint8); mask = np.zeros(no, np.uint8)
    ninl = np.zeros(nt, np.int32); ntr = np.zeros(nt, np.int32); best = np.full(nt, -1, np.int32)
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    check(load().xrsfm_ba_triangulate_tracks(C.byref(o), len(cam_q), _dp(cam_q), _dp(cam_t), nt, ip(trk_ptr), ip(obs_cam), _dp(obs_xy), _dp(points),
                                             status.ctypes.data_as(_c_uint8_p), mask.ctypes.data_as(_c_uint8_p), ip(ninl), ip(ntr), ip(best)),
          "xrsfm_ba_triangulate_tracks")
    return dict(points=points, status=status, inlier_mask=mask, num_inliers=ninl, num_trials=ntr, best_trial=best)


def absolute_pose_options(**overrides) -> CPoseOptions:
    """xrsfm_ba_absolute_pose_options: the settings of the reference's SolvePnP_colmap (max_error for 8 px at a focal length of 800)."""
    o = CPoseOptions()
    load().xrsfm_ba_absolute_pose_options(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def absolute_pose(corr_ptr, xy, points3d, options: CPoseOptions | None = None, frame_max_error=None, frame_seed=None) -> dict:
    """xrsfm_ba_absolute_pose: one P3P LO-RANSAC per frame (correspondences corr_ptr[f] .. corr_ptr[f+1]: normalised image
    coordinates and world points).  q and t of frames whose status is not 1 stay 0 here (the C call leaves them untouched)."""
    o = options if options is not None else absolute_pose_options()
    corr_ptr = np.ascontiguousarray(corr_ptr, np.int32)
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2); points3d = np.ascontiguousarray(points3d, np.float64).reshape(-1, 3)
    if corr_ptr.ndim != 1 or len(corr_ptr) < 1 or len(xy) != len(points3d):
        raise ValueError("absolute_pose: inconsistent array shapes")
    nf, n = len(corr_ptr) - 1, len(xy)
    if nf > 0 and corr_ptr[-1] != n:
        raise ValueError("absolute_pose: corr_ptr[-1] must be the number of correspondences")
    fme = fsd = None
    if frame_max_error is not None:
        fme = np.ascontiguousarray(frame_max_error, np.float64)
        if fme.shape != (nf,):
            raise ValueError("absolute_pose: frame_max_error must have one entry per frame")
    if frame_seed is not None:
        fsd = np.ascontiguousarray(frame_seed, np.uint32)
        if fsd.shape != (nf,):
            raise ValueError("absolute_pose: frame_seed must have one entry per frame")
    q = np.zeros((nf, 4)); t = np.zeros((nf, 3)); status = np.zeros(nf, np.uint8); mask = np.zeros(n, np.uint8)
    ninl = np.zeros(nf, np.int32); ntr = np.zeros(nf, np.int32); best = np.full(nf, -1, np.int32)
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    check(load().xrsfm_ba_absolute_pose(C.byref(o), nf, ip(corr_ptr), _dp(xy), _dp(points3d), _dp(fme) if fme is not None else None,
                                        fsd.ctypes.data_as(C.POINTER(C.c_uint32)) if fsd is not None else None, _dp(q), _dp(t),
                                        status.ctypes.data_as(_c_uint8_p), mask.ctypes.data_as(_c_uint8_p), ip(ninl), ip(ntr), ip(best)),
          "xrsfm_ba_absolute_pose")
    return dict(q=q, t=t, status=status, inlier_mask=mask, num_inliers=ninl, num_trials=ntr, best_trial=best)


def debug_pose_samples(seed: int, n: int, n_trials: int) -> np.ndarray:
    """xrsfm_ba_debug_pose_samples: the sample triples [n_trials][3] of a frame of n correspondences (no GPU)."""
    out = np.zeros((n_trials, 3), np.int32)
    check(load().xrsfm_ba_debug_pose_samples(int(seed), int(n), int(n_trials), out.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_pose_samples")
    return out


def two_view_options(**overrides) -> CTwoViewOptions:
    """xrsfm_ba_two_view_options_default: the settings of the reference's CheckInitFramePair / solve_essential.  min_angle_rad may
    be given as a sequence of up to four angles; n_angles follows it."""
    o = CTwoViewOptions()
    load().xrsfm_ba_two_view_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        if k == "min_angle_rad":
            v = [float(x) for x in v]
            o.n_angles = len(v)
            v = (C.c_double * 4)(*(v + [0.0] * (4 - len(v))))
        setattr(o, k, v)
    return o


class TwoViewResult:
    """The outputs of xrsfm_ba_two_view_init, one entry per pair (status, E [9], q, t, counts [8], accepted, num_trials, best_trial)
    or per match (points, essential_mask, front_mask).  q, t, E and points the call leaves untouched are 0 here."""
    FIELDS = ("status", "E", "q", "t", "points", "essential_mask", "front_mask", "counts", "accepted", "num_trials", "best_trial")

    def __init__(self, match_ptr, **arrays):
        self.match_ptr = match_ptr
        for k in self.FIELDS:
            setattr(self, k, arrays[k])

    def pair(self, p: int) -> dict:
        """the outputs of pair p, the per-match ones cut to its matches"""
        a, b = int(self.match_ptr[p]), int(self.match_ptr[p + 1])
        per_match = ("points", "essential_mask", "front_mask")
        return {k: (getattr(self, k)[a:b] if k in per_match else getattr(self, k)[p]) for k in self.FIELDS}


def two_view_init(match_ptr, xy_a, xy_b, pair_threshold, options: CTwoViewOptions | None = None, pair_seed=None) -> TwoViewResult:
    """xrsfm_ba_two_view_init: one 5-point RANSAC, decomposition and triangulation per candidate pair (matches match_ptr[p] ..
    match_ptr[p+1]: normalised image coordinates in frame 1 and frame 2; pair_threshold[p] = 10 / fx of frame 1)."""
    o = options if options is not None else two_view_options()
    match_ptr = np.ascontiguousarray(match_ptr, np.int32)
    xy_a = np.ascontiguousarray(xy_a, np.float64).reshape(-1, 2); xy_b = np.ascontiguousarray(xy_b, np.float64).reshape(-1, 2)
    if match_ptr.ndim != 1 or len(match_ptr) < 1 or len(xy_a) != len(xy_b):
        raise ValueError("two_view_init: inconsistent array shapes")
    npair, n = len(match_ptr) - 1, len(xy_a)
    if npair > 0 and match_ptr[-1] != n:
        raise ValueError("two_view_init: match_ptr[-1] must be the number of matches")
    th = np.ascontiguousarray(pair_threshold, np.float64)
    if th.shape != (npair,):
        raise ValueError("two_view_init: pair_threshold must have one entry per pair")
    sd = None
    if pair_seed is not None:
        sd = np.ascontiguousarray(pair_seed, np.uint32)
        if sd.shape != (npair,):
            raise ValueError("two_view_init: pair_seed must have one entry per pair")
    r = dict(status=np.zeros(npair, np.uint8), E=np.zeros((npair, 9)), q=np.zeros((npair, 4)), t=np.zeros((npair, 3)), points=np.zeros((n, 3)),
             essential_mask=np.zeros(n, np.uint8), front_mask=np.zeros(n, np.uint8), counts=np.zeros((npair, 8), np.int32),
             accepted=np.zeros(npair, np.uint8), num_trials=np.zeros(npair, np.int32), best_trial=np.full(npair, -1, np.int32))
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    up = lambda a: a.ctypes.data_as(_c_uint8_p)
    check(load().xrsfm_ba_two_view_init(C.byref(o), npair, ip(match_ptr), _dp(xy_a), _dp(xy_b), _dp(th),
                                        sd.ctypes.data_as(C.POINTER(C.c_uint32)) if sd is not None else None, up(r["status"]), _dp(r["E"]), _dp(r["q"]),
                                        _dp(r["t"]), _dp(r["points"]), up(r["essential_mask"]), up(r["front_mask"]), ip(r["counts"]), up(r["accepted"]),
                                        ip(r["num_trials"]), ip(r["best_trial"])), "xrsfm_ba_two_view_init")
    return TwoViewResult(match_ptr, **r)


def first_accepted(order, accepted) -> tuple:
    """FindInitFramePair's two passes (map_initializer.cc:112-136) over the candidates `order` (indices of pairs, best first): all
    candidates at angle 0, then all at angle 1, ...  Returns (pair, angle index), or (-1, -1) when none qualifies."""
    accepted = np.asarray(accepted)
    n_angles = 4
    for a in range(n_angles):
        for p in order:
            if (int(accepted[int(p)]) >> a) & 1:
                return int(p), a
    return -1, -1


def debug_two_view_samples(seed: int, n: int, n_trials: int) -> np.ndarray:
    """xrsfm_ba_debug_two_view_samples: the sample quintuples [n_trials][5] of a pair of n matches (no GPU)."""
    out = np.zeros((n_trials, 5), np.int32)
    check(load().xrsfm_ba_debug_two_view_samples(int(seed), int(n), int(n_trials), out.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_two_view_samples")
    return out


def verify_pairs_options(**overrides) -> CFundOptions:
    """xrsfm_ba_verify_pairs_options: the settings of the reference's SolveFundamnetalCOLMAP and FeatureMatching."""
    o = CFundOptions()
    load().xrsfm_ba_verify_pairs_options(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def verify_pairs(match_ptr, xy_a, xy_b, options: CFundOptions | None = None, pair_max_error=None, pair_seed=None) -> dict:
    """xrsfm_ba_verify_pairs: one 7-point / 8-point LO-RANSAC per matched pair (matches match_ptr[p] .. match_ptr[p+1]: PIXEL
    coordinates in the first and second image).  F of pairs whose status is not 1 stays 0 here (the C call leaves it untouched)."""
    o = options if options is not None else verify_pairs_options()
    match_ptr = np.ascontiguousarray(match_ptr, np.int32)
    xy_a = np.ascontiguousarray(xy_a, np.float64).reshape(-1, 2); xy_b = np.ascontiguousarray(xy_b, np.float64).reshape(-1, 2)
    if match_ptr.ndim != 1 or len(match_ptr) < 1 or len(xy_a) != len(xy_b):
        raise ValueError("verify_pairs: inconsistent array shapes")
    npair, n = len(match_ptr) - 1, len(xy_a)
    if npair > 0 and match_ptr[-1] != n:
        raise ValueError("verify_pairs: match_ptr[-1] must be the number of matches")
    pme = psd = None
    if pair_max_error is not None:
        pme = np.ascontiguousarray(pair_max_error, np.float64)
        if pme.shape != (npair,):
            raise ValueError("verify_pairs: pair_max_error must have one entry per pair")
    if pair_seed is not None:
        psd = np.ascontiguousarray(pair_seed, np.uint32)
        if psd.shape != (npair,):
            raise ValueError("verify_pairs: pair_seed must have one entry per pair")
    r = dict(status=np.zeros(npair, np.uint8), F=np.zeros((npair, 9)), inlier_mask=np.zeros(n, np.uint8), num_inliers=np.zeros(npair, np.int32),
             num_trials=np.zeros(npair, np.int32), best_trial=np.full(npair, -1, np.int32), accepted=np.zeros(npair, np.uint8))
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    up = lambda a: a.ctypes.data_as(_c_uint8_p)
    check(load().xrsfm_ba_verify_pairs(C.byref(o), npair, ip(match_ptr), _dp(xy_a), _dp(xy_b), _dp(pme) if pme is not None else None,
                                       psd.ctypes.data_as(C.POINTER(C.c_uint32)) if psd is not None else None, up(r["status"]), _dp(r["F"]),
                                       up(r["inlier_mask"]), ip(r["num_inliers"]), ip(r["num_trials"]), ip(r["best_trial"]), up(r["accepted"])),
          "xrsfm_ba_verify_pairs")
    return r


def verified_matches(result: dict, match_ptr, matches) -> tuple:
    """FeatureMatching after the verification (feature_processing.cc:291-305): the pairs with accepted != 0 keep their inlier
    matches (ExtractInlierMatches), every other pair is dropped.  `matches` has one row per match (any columns: feature indices,
    coordinates).  Returns (kept pair indices, the kept rows, their match_ptr): what two_view_init takes."""
    match_ptr = np.asarray(match_ptr, np.int64)
    matches = np.asarray(matches)
    mask = np.asarray(result["inlier_mask"], bool)
    if len(matches) != len(mask) or len(match_ptr) != len(result["accepted"]) + 1:
        raise ValueError("verified_matches: inconsistent array shapes")
    kept = np.flatnonzero(np.asarray(result["accepted"]) != 0)
    rows = [np.arange(match_ptr[p], match_ptr[p + 1])[mask[match_ptr[p]:match_ptr[p + 1]]] for p in kept]
    new_ptr = np.zeros(len(kept) + 1, np.int32)
    if len(kept):
        new_ptr[1:] = np.cumsum([len(r) for r in rows])
    sel = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    return kept, matches[sel], new_ptr


def debug_fund_samples(seed: int, n: int, n_trials: int) -> np.ndarray:
    """xrsfm_ba_debug_fund_samples: the sample septuples [n_trials][7] of a pair of n matches (no GPU)."""
    out = np.zeros((n_trials, 7), np.int32)
    check(load().xrsfm_ba_debug_fund_samples(int(seed), int(n), int(n_trials), out.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_fund_samples")
    return out


def match_options(**overrides) -> CMatchOptions:
    """xrsfm_ba_match_options_default: the settings of the reference's FeatureMatching."""
    o = CMatchOptions()
    load().xrsfm_ba_match_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def _desc2d(desc) -> np.ndarray:
    d = np.ascontiguousarray(desc, np.uint8)
    return d.reshape(d.size // MATCH_DIM if d.size % MATCH_DIM == 0 else -1, MATCH_DIM)


def match_descriptors(desc_ptr, desc, pair_a, pair_b, options: CMatchOptions | None = None) -> dict:
    """xrsfm_ba_match_descriptors: the SIFT matches of every pair (frame pair_a[p] against frame pair_b[p]; the descriptors of frame f
    are rows desc_ptr[f] .. desc_ptr[f+1] of the uint8 array desc [n][128]).  Returns match_ptr [n_pairs+1] (int64), matches
    [match_ptr[-1]][2] (feature index in a, in b), num_row and num_col [n_pairs]."""
    o = options if options is not None else match_options()
    desc_ptr = np.ascontiguousarray(desc_ptr, np.int64)
    desc = _desc2d(desc)
    pair_a = np.ascontiguousarray(pair_a, np.int32); pair_b = np.ascontiguousarray(pair_b, np.int32)
    if desc_ptr.ndim != 1 or len(desc_ptr) < 1 or pair_a.ndim != 1 or pair_a.shape != pair_b.shape:
        raise ValueError("match_descriptors: inconsistent array shapes")
    if desc_ptr[-1] != len(desc):
        raise ValueError("match_descriptors: desc_ptr[-1] must be the number of descriptors")
    nf, npair = len(desc_ptr) - 1, len(pair_a)
    n = np.minimum(np.diff(desc_ptr), max(int(o.max_features), 0))
    ok = npair > 0 and nf > 0 and pair_a.min() >= 0 and pair_a.max() < nf
    cap = int(n[pair_a].sum()) if ok else 0                  # (an index out of range is the library's to refuse)
    mp = np.zeros(npair + 1, np.int64); m = np.zeros((cap, 2), np.int32)
    r = dict(num_row=np.zeros(npair, np.int32), num_col=np.zeros(npair, np.int32))
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    check(load().xrsfm_ba_match_descriptors(C.byref(o), nf, lp(desc_ptr), desc.ctypes.data_as(_c_uint8_p), npair, ip(pair_a), ip(pair_b), cap, lp(mp), ip(m),
                                            ip(r["num_row"]), ip(r["num_col"])), "xrsfm_ba_match_descriptors")
    r["match_ptr"] = mp
    r["matches"] = m[:int(mp[-1])].copy()
    return r


def matched_points(result: dict, kp_ptr, keypoints_xy, pair_a, pair_b) -> tuple:
    """The coordinates of the matches of match_descriptors: keypoints_xy [n][2] holds the keypoints of frame f at rows kp_ptr[f] ..
    kp_ptr[f+1], in the order of its descriptors.  Returns (xy_a, xy_b), one row per match: what verify_pairs takes together with
    result["match_ptr"]."""
    kp_ptr = np.asarray(kp_ptr, np.int64)
    xy = np.ascontiguousarray(keypoints_xy, np.float64).reshape(-1, 2)
    mp, m = np.asarray(result["match_ptr"], np.int64), np.asarray(result["matches"], np.int64).reshape(-1, 2)
    pair_a, pair_b = np.asarray(pair_a, np.int64), np.asarray(pair_b, np.int64)
    if len(mp) != len(pair_a) + 1 or len(pair_a) != len(pair_b) or (len(mp) and mp[-1] != len(m)):
        raise ValueError("matched_points: inconsistent array shapes")
    per = np.diff(mp)
    return xy[np.repeat(kp_ptr[pair_a], per) + m[:, 0]], xy[np.repeat(kp_ptr[pair_b], per) + m[:, 1]]


def quantize_descriptors(float_desc) -> np.ndarray:
    """SetDescriptors(float) of the reference (SiftMatchCU.cpp:131-135): unit-norm float descriptors to uint8 by int(512 d + 0.5).
    The reference stores the int into an unsigned char; values that do not fit are refused here."""
    q = (512.0 * np.asarray(float_desc, np.float32) + np.float32(0.5)).astype(np.int32)
    if q.size and (q.min() < 0 or q.max() > 255):
        raise ValueError("quantize_descriptors: a component outside [0, 255 / 512]")
    return q.astype(np.uint8)


def debug_match_table() -> np.ndarray:
    """xrsfm_ba_debug_match_table: dist(0 .. 2^18) as the library builds it (no GPU)."""
    out = np.zeros(MATCH_TABLE_SIZE, np.float32)
    check(load().xrsfm_ba_debug_match_table(out.ctypes.data_as(C.POINTER(C.c_float))), "xrsfm_ba_debug_match_table")
    return out


def debug_match_top2(desc_a, desc_b) -> tuple:
    """xrsfm_ba_debug_match_top2: (row_top [n_a][3], col_top [n_b][3]), the triples (best, idx, next) of one pair."""
    a, b = _desc2d(desc_a), _desc2d(desc_b)
    rt, ct = np.zeros((len(a), 3), np.int32), np.zeros((len(b), 3), np.int32)
    check(load().xrsfm_ba_debug_match_top2(len(a), a.ctypes.data_as(_c_uint8_p), len(b), b.ctypes.data_as(_c_uint8_p), rt.ctypes.data_as(_c_int32_p),
                                           ct.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_match_top2")
    return rt, ct


def debug_pack(problem: ProblemArrays) -> dict:
    """Host-side packing statistics and the slot -> observation map (works without a GPU)."""
    stats = np.zeros(8, np.int32)
    slot_obs = np.full(problem.n_obs + 64 * (problem.n_points + 1), -2, np.int32)
    cs = problem.c_struct()
    check(load().xrsfm_ba_debug_pack(C.byref(cs), stats.ctypes.data_as(_c_int32_p), slot_obs.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_pack")
    keys = ("tiles", "slots", "items", "regular_tiles", "long_items", "cam_entries", "longest_track", "active_points")
    out = dict(zip(keys, (int(v) for v in stats)))
    out["slot_obs"] = slot_obs[:out["slots"]].copy()
    return out


def debug_device_pack_check(problem: ProblemArrays) -> tuple:
    """Device-side packing (large problems) against the host packing: (field, index) of the first difference, (0, -1) when every
    array is identical, (-100, -1) when the device path declines the problem.  Needs a GPU."""
    lib = load()
    lib.xrsfm_ba_debug_device_pack_check.argtypes = [C.POINTER(CProblem), _c_int32_p, _c_int32_p]
    lib.xrsfm_ba_debug_device_pack_check.restype = C.c_int
    f = np.zeros(1, np.int32); i = np.zeros(1, np.int32)
    cs = problem.c_struct()
    check(lib.xrsfm_ba_debug_device_pack_check(C.byref(cs), f.ctypes.data_as(_c_int32_p), i.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_device_pack_check")
    return int(f[0]), int(i[0])


def debug_chol_plan(problem: ProblemArrays) -> dict:
    """Host-side plan of the Cholesky path: tiles, elimination-tree levels, ordering (works without a GPU)."""
    stats = np.zeros(8, np.int32)
    off = np.zeros(max(problem.n_cams, 1), np.int32)
    facts = np.zeros(16, np.int32)
    cs = problem.c_struct()
    check(load().xrsfm_ba_debug_chol_plan(C.byref(cs), stats.ctypes.data_as(_c_int32_p), off.ctypes.data_as(_c_int32_p),
                                          facts.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_chol_plan")
    keys = ("tiles", "levels", "ordering", "hubs", "band", "blocks", "level_schedule", "tiles_nz")
    out = dict(zip(keys, (int(v) for v in stats)))
    out["lookahead"] = (out["level_schedule"] >> 1) & 1      # panel schedule with partial products on a second stream (ba_plan.h)
    out["level_schedule"] &= 1
    out["cam_offset"] = off[:problem.n_cams].copy()
    out["facts"] = _facts(facts)       # the schedule facts of debug_reduced_system (packed storage and the forms from the environment)
    return out


def refine_pose_options(**overrides) -> "COptions":
    """Settings of the reference's pose refinement (pnp.cc:57-60): Ceres defaults, 10 iterations."""
    o = COptions()
    load().xrsfm_ba_refine_pose_options(C.byref(o))
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


def refine_pose(model: int, intr_params, points3d, uv, q, t, inlier_mask=None, options=None):
    """xrsfm_ba_refine_pose: returns (q, t, summary); inputs are not modified."""
    prm = np.zeros(8); prm[:len(intr_params)] = np.asarray(intr_params, float)[:8]
    P = np.ascontiguousarray(points3d, float).reshape(-1, 3); UV = np.ascontiguousarray(uv, float).reshape(-1, 2)
    q = np.array(q, float).reshape(4).copy(); t = np.array(t, float).reshape(3).copy()
    mask = None if inlier_mask is None else np.ascontiguousarray(inlier_mask, np.uint8)
    s = CSummary()
    check(load().xrsfm_ba_refine_pose(C.byref(options) if options is not None else None, int(model), _dp(prm), P.shape[0], _dp(P), _dp(UV),
                                      mask.ctypes.data_as(_c_uint8_p) if mask is not None else None, _dp(q), _dp(t), C.byref(s)),
          "xrsfm_ba_refine_pose")
    return q, t, s


def refine_poses(models, intr_params, frames, q, t, options=None):
    """xrsfm_ba_refine_poses: `frames` is a list of (points3d [n,3], uv [n,2], inlier_mask or None) per frame; models
    [n_frames], intr_params [n_frames][<=8], q [n_frames][4], t [n_frames][3].  Returns (q, t, [summary per frame])."""
    nf = len(frames)
    prm = np.zeros((nf, 8))
    for f in range(nf):
        v = np.asarray(intr_params[f], float)[:8]; prm[f, :len(v)] = v
    corr_ptr = np.zeros(nf + 1, np.int32)
    for f in range(nf):
        corr_ptr[f + 1] = corr_ptr[f] + np.asarray(frames[f][0]).reshape(-1, 3).shape[0]
    P = np.ascontiguousarray(np.vstack([np.asarray(fr[0], float).reshape(-1, 3) for fr in frames]) if nf else np.zeros((0, 3)))
    UV = np.ascontiguousarray(np.vstack([np.asarray(fr[1], float).reshape(-1, 2) for fr in frames]) if nf else np.zeros((0, 2)))
    any_mask = any(fr[2] is not None for fr in frames)
    mask = None
    if any_mask:
        mask = np.ascontiguousarray(np.concatenate([np.ones(np.asarray(fr[0]).reshape(-1, 3).shape[0], np.uint8) if fr[2] is None
                                                    else np.asarray(fr[2], np.uint8) for fr in frames]))
    q = np.array(q, float).reshape(nf, 4).copy(); t = np.array(t, float).reshape(nf, 3).copy()
    mdl = np.ascontiguousarray(models, np.int32)
    sums = (CSummary * max(nf, 1))()
    check(load().xrsfm_ba_refine_poses(C.byref(options) if options is not None else None, nf, mdl.ctypes.data_as(_c_int32_p), _dp(prm),
                                       corr_ptr.ctypes.data_as(_c_int32_p), _dp(P), _dp(UV),
                                       mask.ctypes.data_as(_c_uint8_p) if mask is not None else None, _dp(q), _dp(t), sums),
          "xrsfm_ba_refine_poses")
    return q, t, [sums[f] for f in range(nf)]


def pose_graph_solve(rot_q, pos, scale, edges, weight_o=0.0, scale_costs=(), pos_const=None, scale_const=None, scale_lower=None,
                     **opt_overrides):
    """xrsfm_pg_solve (host code).  edges: dict(a, b, sa, sb, q_mea [n,4], p_mea [n,3]); scale_costs:
    iterable of (sa, sb, s12).  Returns (pos, scale, summary); inputs are not modified."""
    rot_q = np.ascontiguousarray(rot_q, float); pos = np.array(pos, float, copy=True); scale = np.array(scale, float, copy=True)
    keep = [rot_q, pos, scale]
    p = CPgProblem()
    p.n_frames, p.n_scales = rot_q.shape[0], scale.shape[0]
    p.rot_q, p.pos, p.scale = _dp(rot_q), _dp(pos), _dp(scale)

    def u8(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, np.uint8); keep.append(a); return a.ctypes.data_as(_c_uint8_p)

    def i32(a):
        a = np.ascontiguousarray(a, np.int32); keep.append(a); return a.ctypes.data_as(_c_int32_p)

    def f64(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a, float); keep.append(a); return _dp(a)

    p.pos_const, p.scale_const, p.scale_lower = u8(pos_const), u8(scale_const), f64(scale_lower)
    p.n_edges = len(edges["a"])
    p.edge_a, p.edge_b, p.edge_sa, p.edge_sb = i32(edges["a"]), i32(edges["b"]), i32(edges["sa"]), i32(edges["sb"])
    p.edge_q_mea, p.edge_p_mea = f64(edges["q_mea"]), f64(edges["p_mea"])
    p.weight_o = float(weight_o)
    sc = list(scale_costs)
    p.n_scale_costs = len(sc)
    p.sc_a, p.sc_b, p.sc_s12 = i32([c[0] for c in sc]), i32([c[1] for c in sc]), f64([c[2] for c in sc])
    o = CPgOptions()
    load().xrsfm_pg_default_options(C.byref(o))
    for k, v in opt_overrides.items():
        setattr(o, k, v)
    s = CPgSummary()
    check(load().xrsfm_pg_solve(C.byref(o), C.byref(p), C.byref(s)), "xrsfm_pg_solve")
    return pos, scale, s


def tag_refine(frame_q, frame_t, tag_corners, tag_obs_tag, tag_obs_frame, tag_obs_xy, tag_length, points=None, obs_frame=None,
               obs_pt=None, obs_xy=None, stages=2, tag_q=None, tag_t=None, scale=1.0, scale_lower=0.2, **opt_overrides):
    """xrsfm_tag_refine (host code): the two solves of tag_refine (tag_extract.hpp:193-265).
    Returns dict(scale, tag_q, tag_t, tag_corners, points, summaries); inputs are not modified."""
    keep = []

    def f64(a, copy=False):
        a = np.array(a, float, copy=True) if copy else np.ascontiguousarray(a, float)
        keep.append(a); return a

    def i32(a):
        a = np.ascontiguousarray(a, np.int32); keep.append(a); return a

    frame_q, frame_t = f64(frame_q), f64(frame_t)
    corners = f64(tag_corners, copy=True).reshape(-1, 4, 3)
    n_tags = corners.shape[0]
    tq = f64(np.tile([0.0, 0.0, 0.0, 1.0], (n_tags, 1)) if tag_q is None else tag_q, copy=True)
    tt = f64(np.zeros((n_tags, 3)) if tag_t is None else tag_t, copy=True)
    p = CTagProblem()
    p.n_frames, p.frame_q, p.frame_t = frame_q.shape[0], _dp(frame_q), _dp(frame_t)
    p.n_tags, p.tag_length, p.tag_corners, p.tag_q, p.tag_t = n_tags, float(tag_length), _dp(corners), _dp(tq), _dp(tt)
    p.scale, p.scale_lower = float(scale), float(scale_lower)
    ot, of, oxy = i32(tag_obs_tag), i32(tag_obs_frame), f64(tag_obs_xy)
    p.n_tag_obs, p.tag_obs_tag, p.tag_obs_frame, p.tag_obs_xy = ot.shape[0], ot.ctypes.data_as(_c_int32_p), of.ctypes.data_as(_c_int32_p), _dp(oxy)
    pts = None
    if points is not None:
        pts = f64(points, copy=True)
        a, b, c = i32(obs_frame), i32(obs_pt), f64(obs_xy)
        p.n_points, p.n_obs, p.points = pts.shape[0], a.shape[0], _dp(pts)
        p.obs_frame, p.obs_pt, p.obs_xy = a.ctypes.data_as(_c_int32_p), b.ctypes.data_as(_c_int32_p), _dp(c)
    o = CPgOptions()
    load().xrsfm_tag_default_options(C.byref(o))
    for k, v in opt_overrides.items():
        setattr(o, k, v)
    sums = (CPgSummary * 2)()
    check(load().xrsfm_tag_refine(C.byref(o), C.byref(p), int(stages), sums), "xrsfm_tag_refine")
    return dict(scale=p.scale, tag_q=tq, tag_t=tt, tag_corners=corners, points=pts, summaries=[sums[i] for i in range(stages)])


def debug_gram_schedule(n_cams: int) -> dict:
    """Schedule of 4x4 result blocks of a Gram tile of n_cams cameras (works without a GPU): instructions used by the 4x4 form (0 = the tile
    takes 16x16 result tiles), instructions of the full schedule, and its (row group, column group) blocks, four per instruction."""
    n = C.c_int32(0); na = C.c_int32(0)
    ent = np.zeros(128, np.uint16)
    f = load().xrsfm_ba_debug_gram_schedule
    f.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint16)]
    f.restype = C.c_int
    check(f(int(n_cams), C.byref(n), C.byref(na), ent.ctypes.data_as(C.POINTER(C.c_uint16))), "xrsfm_ba_debug_gram_schedule")
    e = ent[:4 * na.value]
    return dict(n_inst=n.value, n_inst_all=na.value, blocks=[(int(v & 255), int(v >> 8)) for v in e])


def debug_sgroup(problem: ProblemArrays, G: int = 4) -> dict:
    """Tile groups of the S assembly's merged Gram launch on the host-side packing (works without a GPU): per launch position its
    tile and code (index in run | length << 4); per tile L and the cameras / cidx of its first slots; the compact camera pointers."""
    st = debug_pack(problem)
    nt, ns, nc = max(st["tiles"], 1), max(st["slots"], 1), int(problem.n_cams)
    stats = np.zeros(3, np.int32)
    ptile = np.zeros(nt, np.int32); pcode = np.zeros(nt, np.int32); tstride = np.zeros(nt, np.int32)
    tcams = np.zeros((nt, 4), np.int32); tcidx = np.zeros((nt, 4), np.int32); cptr = np.zeros(nc + 1, np.int32)
    cs = problem.c_struct()
    p = lambda a: a.ctypes.data_as(_c_int32_p)
    check(load().xrsfm_ba_debug_sgroup(C.byref(cs), int(G), p(stats), p(ptile), p(pcode), p(tstride), p(tcams), p(tcidx), p(cptr)),
          "xrsfm_ba_debug_sgroup")
    n = int(stats[0])
    return dict(positions=n, cam_entries=int(stats[1]), cam_entries_kept=int(stats[2]), pos_tile=ptile[:n], pos_code=pcode[:n],
                tile_stride=tstride[:st["tiles"]], tile_cams=tcams[:st["tiles"]], tile_cidx=tcidx[:st["tiles"]], cam_ptr_s=cptr,
                gram=debug_pack_gram(problem))


def debug_pack_gram(problem: ProblemArrays) -> dict:
    """Gram tiles and S-assembly item classes of the host-side packing (works without a GPU)."""
    st = debug_pack(problem)
    stats = np.zeros(8, np.int32)
    ncam = np.zeros(max(st["tiles"], 1), np.int32); cidx = np.zeros(max(st["slots"], 1), np.uint8); cpg = np.zeros(max(st["slots"], 1), np.int32)
    cs = problem.c_struct()
    check(load().xrsfm_ba_debug_pack_gram(C.byref(cs), stats.ctypes.data_as(_c_int32_p), ncam.ctypes.data_as(_c_int32_p),
                                          cidx.ctypes.data_as(_c_uint8_p), cpg.ctypes.data_as(_c_int32_p)), "xrsfm_ba_debug_pack_gram")
    keys = ("gram_tiles", "table_cells", "cam_entries_g", "max_cams", "items_small", "items_big", "items_other", "block_writes")
    out = dict(zip(keys, (int(v) for v in stats)))
    out.update(tile_ncam=ncam[:st["tiles"]], slot_cidx=cidx[:st["slots"]], slot_campos_g=cpg[:st["slots"]], slot_obs=st["slot_obs"],
               items=st["items"], long_items=st["long_items"])
    return out


def sift_options(**overrides) -> CSiftOptions:
    """xrsfm_ba_sift_options_default: the settings of the reference's SiftExtractor."""
    o = CSiftOptions()
    load().xrsfm_ba_sift_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def sift_geometry(width: int, height: int, options: CSiftOptions | None = None) -> list:
    """[(stored width, height)] of the octaves of a width x height image (include/xrsfm_ba.h)."""
    o = options if options is not None else sift_options()
    w0, h0 = (width & ~3) << (1 if o.first_octave < 0 else 0), height << (1 if o.first_octave < 0 else 0)
    n = min(int(o.num_octaves), max(1, min(w0, h0).bit_length() - 1 - 3))
    return [(((w0 >> k) + 3) // 4 * 4, h0 >> k) for k in range(n)]


def _grey(image) -> np.ndarray:
    a = np.asarray(image)
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError("an image must be a 2-D uint8 array")
    return np.ascontiguousarray(a)


def detect_keypoints(images, options: CSiftOptions | None = None, capacity: int | None = None) -> list:
    """xrsfm_ba_detect_keypoints on a list of 2-D uint8 arrays (any sizes): per image a dict of keys [n][4] (X, Y, S, 0), loc [n][4]
    (octave, level, row, col), sign [n] and level_count [num_octaves * 3] (before the budget).  capacity: of the output arrays;
    by default the call is repeated once with the size the library names."""
    o = options if options is not None else sift_options()
    imgs = [_grey(a) for a in images]
    n = len(imgs)
    w = np.array([a.shape[1] for a in imgs], np.int32); h = np.array([a.shape[0] for a in imgs], np.int32)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([a.size for a in imgs])
    pix = np.concatenate([a.ravel() for a in imgs]) if n else np.zeros(0, np.uint8)
    nl = max(int(o.num_octaves), 0) * 3
    lc = np.zeros((n, nl), np.int32); kp = np.zeros(n + 1, np.int64)
    lib = load()

    def run(cap):
        k = np.zeros((cap, 4), np.float32); l = np.zeros((cap, 4), np.int32); s = np.zeros(cap, np.int8)
        code = lib.xrsfm_ba_detect_keypoints(C.byref(o), n, w.ctypes.data_as(_c_int32_p), h.ctypes.data_as(_c_int32_p), ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                             pix.ctypes.data_as(_c_uint8_p), cap, kp.ctypes.data_as(C.POINTER(C.c_int64)), k.ctypes.data_as(C.POINTER(C.c_float)),
                                             l.ctypes.data_as(_c_int32_p), s.ctypes.data_as(C.POINTER(C.c_int8)), lc.ctypes.data_as(_c_int32_p))
        return code, k, l, s
    # (the budget lets an image exceed max_num_features by part of one level only)
    first = max(n, 1) * min(max(int(o.max_num_features), 0) + 4096, 65536) if capacity is None else int(capacity)
    code, k, l, s = run(first)
    if code == EINVAL and capacity is None and n > 0 and kp[-1] > first:
        code, k, l, s = run(int(kp[-1]))
    check(code, "xrsfm_ba_detect_keypoints")
    return [dict(keys=k[kp[i]:kp[i + 1]].copy(), loc=l[kp[i]:kp[i + 1]].copy(), sign=s[kp[i]:kp[i + 1]].copy(), level_count=lc[i].copy()) for i in range(n)]


def debug_sift_taps(sigma: float) -> np.ndarray:
    """xrsfm_ba_debug_sift_taps: the normalised taps of one sigma, cut to their width (no GPU)."""
    t = np.zeros(SIFT_MAX_TAPS, np.float32)
    wd = C.c_int32(0)
    check(load().xrsfm_ba_debug_sift_taps(float(sigma), t.ctypes.data_as(C.POINTER(C.c_float)), C.byref(wd)), "xrsfm_ba_debug_sift_taps")
    return t[:wd.value].copy()


def debug_sift_levels(image, octave: int, options: CSiftOptions | None = None) -> tuple:
    """xrsfm_ba_debug_sift_levels: (gauss [6][h][w], dog [5][h][w]) of one octave of one image."""
    o = options if options is not None else sift_options()
    a = _grey(image)
    geo = sift_geometry(a.shape[1], a.shape[0], o)
    if not 0 <= octave < len(geo):
        raise ValueError("debug_sift_levels: the image has no such octave")
    ws, hs = geo[octave]
    g = np.zeros((6, hs, ws), np.float32); d = np.zeros((5, hs, ws), np.float32)
    check(load().xrsfm_ba_debug_sift_levels(C.byref(o), a.shape[1], a.shape[0], a.ctypes.data_as(_c_uint8_p), octave, g.ctypes.data_as(C.POINTER(C.c_float)),
                                            d.ctypes.data_as(C.POINTER(C.c_float))), "xrsfm_ba_debug_sift_levels")
    return g, d


def debug_sift_offsets(image, options: CSiftOptions | None = None) -> tuple:
    """xrsfm_ba_debug_sift_offsets: (loc [n][4], offsets [n][4] = (sign, dx, dy, ds)) of one image, in the order of detect_keypoints."""
    o = options if options is not None else sift_options()
    a = _grey(image)
    n = C.c_int64(0)
    cap = 4096
    for _ in range(2):
        l = np.zeros((cap, 4), np.int32); f = np.zeros((cap, 4), np.float32)
        code = load().xrsfm_ba_debug_sift_offsets(C.byref(o), a.shape[1], a.shape[0], a.ctypes.data_as(_c_uint8_p), cap, C.byref(n), l.ctypes.data_as(_c_int32_p),
                                                  f.ctypes.data_as(C.POINTER(C.c_float)))
        if code == EINVAL and n.value > cap:
            cap = int(n.value)
            continue
        break
    check(code, "xrsfm_ba_debug_sift_offsets")
    return l[:n.value].copy(), f[:n.value].copy()


def sift_desc_options(**overrides) -> CSiftDescOptions:
    """xrsfm_ba_sift_desc_options_default: one orientation per keypoint, not upright."""
    o = CSiftDescOptions()
    load().xrsfm_ba_sift_desc_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def extract_features(images, options: CSiftOptions | None = None, desc_options: CSiftDescOptions | None = None, capacity: int | None = None,
                     floats: bool = True) -> list:
    """xrsfm_ba_extract_features on a list of 2-D uint8 arrays: per image the dict of detect_keypoints (keys[:, 3] now the
    orientation) plus desc [n][128] uint8 and desc_float [n][128] (None with floats=False)."""
    o = options if options is not None else sift_options()
    do = desc_options if desc_options is not None else sift_desc_options()
    imgs = [_grey(a) for a in images]
    n = len(imgs)
    w = np.array([a.shape[1] for a in imgs], np.int32); h = np.array([a.shape[0] for a in imgs], np.int32)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([a.size for a in imgs])
    pix = np.concatenate([a.ravel() for a in imgs]) if n else np.zeros(0, np.uint8)
    nl = max(int(o.num_octaves), 0) * 3
    lc = np.zeros((n, nl), np.int32); kp = np.zeros(n + 1, np.int64)
    lib = load()

    def run(cap):
        k = np.zeros((cap, 4), np.float32); l = np.zeros((cap, 4), np.int32); s = np.zeros(cap, np.int8)
        d = np.zeros((cap, 128), np.uint8); f = np.zeros((cap, 128), np.float32) if floats else None
        code = lib.xrsfm_ba_extract_features(C.byref(o), C.byref(do), n, w.ctypes.data_as(_c_int32_p), h.ctypes.data_as(_c_int32_p), ptr.ctypes.data_as(C.POINTER(C.c_int64)),
                                             pix.ctypes.data_as(_c_uint8_p), cap, kp.ctypes.data_as(C.POINTER(C.c_int64)), k.ctypes.data_as(C.POINTER(C.c_float)),
                                             l.ctypes.data_as(_c_int32_p), s.ctypes.data_as(C.POINTER(C.c_int8)), d.ctypes.data_as(_c_uint8_p),
                                             f.ctypes.data_as(C.POINTER(C.c_float)) if floats else None, lc.ctypes.data_as(_c_int32_p))
        return code, k, l, s, d, f
    first = max(n, 1) * min(max(int(o.max_num_features), 0) + 4096, 65536) if capacity is None else int(capacity)
    code, k, l, s, d, f = run(first)
    if code == EINVAL and capacity is None and n > 0 and kp[-1] > first:
        code, k, l, s, d, f = run(int(kp[-1]))
    check(code, "xrsfm_ba_extract_features")
    return [dict(keys=k[kp[i]:kp[i + 1]].copy(), loc=l[kp[i]:kp[i + 1]].copy(), sign=s[kp[i]:kp[i + 1]].copy(), level_count=lc[i].copy(),
                 desc=d[kp[i]:kp[i + 1]].copy(), desc_float=f[kp[i]:kp[i + 1]].copy() if floats else None) for i in range(n)]


def feature_frames(results) -> tuple:
    """(desc [N][128] uint8, desc_ptr [n + 1], keypoints_xy [N][2]) of extract_features' results, ready for match_descriptors and
    matched_points."""
    ptr = np.zeros(len(results) + 1, np.int64)
    ptr[1:] = np.cumsum([len(r["desc"]) for r in results])
    desc = np.concatenate([r["desc"] for r in results]) if results else np.zeros((0, 128), np.uint8)
    xy = np.concatenate([r["keys"][:, :2] for r in results]) if results else np.zeros((0, 2), np.float32)
    return np.ascontiguousarray(desc.reshape(-1, 128)), ptr, np.ascontiguousarray(xy.reshape(-1, 2).astype(np.float32))


_default_match_options = match_options      # (frames_match has a parameter of that name)


class Frames:
    """A device-resident frame set (xrsfm_ba_frames): the features of n frames on device 0, immutable, for one thread at a time.
    A context manager; close() and __del__ give its device memory back."""

    def __init__(self, handle, from_images: bool, num_levels: int = 0):
        self.handle, self.from_images, self.num_levels = handle, from_images, num_levels

    def close(self):
        if getattr(self, "handle", None):
            load().xrsfm_ba_frames_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _h(self):
        if not self.handle:
            raise RuntimeError("the frame set is closed")
        return self.handle


def frames_create(key_ptr, keys, desc) -> Frames:
    """xrsfm_ba_frames_create: a set from existing features (keys [N][4] float32 as extract_features returns them, or [N][2]: x, y;
    desc [N][128] uint8; frame f owns rows key_ptr[f] .. key_ptr[f+1])."""
    key_ptr = np.ascontiguousarray(key_ptr, np.int64)
    k = np.asarray(keys, np.float32)
    k = k.reshape(-1, 4) if k.ndim == 1 else k
    if k.ndim != 2 or k.shape[1] not in (2, 4) or key_ptr.ndim != 1 or len(key_ptr) < 1:
        raise ValueError("frames_create: inconsistent array shapes")
    if k.shape[1] == 2:
        k = np.concatenate([k, np.zeros((len(k), 2), np.float32)], axis=1)
    k = np.ascontiguousarray(k, np.float32)
    d = _desc2d(desc)
    if len(k) != len(d) or key_ptr[-1] != len(d):
        raise ValueError("frames_create: key_ptr[-1] must be the number of key points and of descriptors")
    h = C.c_void_p()
    check(load().xrsfm_ba_frames_create(len(key_ptr) - 1, key_ptr.ctypes.data_as(C.POINTER(C.c_int64)), k.ctypes.data_as(C.POINTER(C.c_float)),
                                        d.ctypes.data_as(_c_uint8_p), C.byref(h)), "xrsfm_ba_frames_create")
    return Frames(h, False)


def frames_from_images(images, options: CSiftOptions | None = None, desc_options: CSiftDescOptions | None = None) -> Frames:
    """xrsfm_ba_frames_from_images: extract_features on a list of 2-D uint8 arrays straight into a set."""
    o = options if options is not None else sift_options()
    do = desc_options if desc_options is not None else sift_desc_options()
    imgs = [_grey(a) for a in images]
    n = len(imgs)
    w = np.array([a.shape[1] for a in imgs], np.int32); h = np.array([a.shape[0] for a in imgs], np.int32)
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([a.size for a in imgs])
    pix = np.concatenate([a.ravel() for a in imgs]) if n else np.zeros(0, np.uint8)
    hd = C.c_void_p()
    check(load().xrsfm_ba_frames_from_images(C.byref(o), C.byref(do), n, w.ctypes.data_as(_c_int32_p), h.ctypes.data_as(_c_int32_p),
                                             ptr.ctypes.data_as(C.POINTER(C.c_int64)), pix.ctypes.data_as(_c_uint8_p), C.byref(hd)), "xrsfm_ba_frames_from_images")
    return Frames(hd, True, max(int(o.num_octaves), 0) * 3)


def frames_info(frames: Frames) -> dict:
    """xrsfm_ba_frames_info: n_frames, key_ptr [n_frames + 1] and the device bytes the set holds."""
    n = C.c_int32(0); b = C.c_uint64(0)
    lib = load()
    check(lib.xrsfm_ba_frames_info(frames._h(), C.byref(n), None, C.byref(b)), "xrsfm_ba_frames_info")
    kp = np.zeros(n.value + 1, np.int64)
    check(lib.xrsfm_ba_frames_info(frames._h(), None, kp.ctypes.data_as(C.POINTER(C.c_int64)), None), "xrsfm_ba_frames_info")
    return dict(n_frames=int(n.value), key_ptr=kp, device_bytes=int(b.value))


def frames_download(frames: Frames) -> list:
    """xrsfm_ba_frames_download: per frame the dict of extract_features (keys, desc; for a set made from images also loc, sign and
    level_count; desc_float is not held: None)."""
    info = frames_info(frames)
    kp, n = info["key_ptr"], info["n_frames"]
    cap = int(kp[-1])
    k = np.zeros((cap, 4), np.float32); d = np.zeros((cap, 128), np.uint8)
    img = frames.from_images
    l = np.zeros((cap, 4), np.int32) if img else None
    s = np.zeros(cap, np.int8) if img else None
    lc = np.zeros((n, frames.num_levels), np.int32) if img else None
    check(load().xrsfm_ba_frames_download(frames._h(), cap, k.ctypes.data_as(C.POINTER(C.c_float)), d.ctypes.data_as(_c_uint8_p),
                                          l.ctypes.data_as(_c_int32_p) if img else None, s.ctypes.data_as(C.POINTER(C.c_int8)) if img else None,
                                          lc.ctypes.data_as(_c_int32_p) if img else None), "xrsfm_ba_frames_download")
    out = []
    for i in range(n):
        r = dict(keys=k[kp[i]:kp[i + 1]].copy(), desc=d[kp[i]:kp[i + 1]].copy())
        if img:
            r.update(loc=l[kp[i]:kp[i + 1]].copy(), sign=s[kp[i]:kp[i + 1]].copy(), level_count=lc[i].copy(), desc_float=None)
        out.append(r)
    return out


def frames_match(frames: Frames, pair_a, pair_b, match_options: CMatchOptions | None = None, fund_options: CFundOptions | None = None,
                 pair_max_error=None, pair_seed=None) -> dict:
    """xrsfm_ba_frames_match: FeatureMatching on a resident set.  Returns the dict of match_descriptors (match_ptr, matches, num_row,
    num_col) and, with fund_options, the keys of verify_pairs (status, F, inlier_mask, num_inliers, num_trials, best_trial,
    accepted) on the matched key points: verified_matches takes it with its own match_ptr and matches."""
    mo = match_options if match_options is not None else _default_match_options()
    pair_a = np.ascontiguousarray(pair_a, np.int32); pair_b = np.ascontiguousarray(pair_b, np.int32)
    if pair_a.ndim != 1 or pair_a.shape != pair_b.shape:
        raise ValueError("frames_match: inconsistent array shapes")
    info = frames_info(frames)
    nf, npair = info["n_frames"], len(pair_a)
    n = np.minimum(np.diff(info["key_ptr"]), max(int(mo.max_features), 0))
    ok = npair > 0 and nf > 0 and pair_a.min() >= 0 and pair_a.max() < nf
    cap = int(n[pair_a].sum()) if ok else 0                  # (an index out of range is the library's to refuse)
    mp = np.zeros(npair + 1, np.int64); m = np.zeros((cap, 2), np.int32)
    r = dict(num_row=np.zeros(npair, np.int32), num_col=np.zeros(npair, np.int32))
    ip = lambda a: a.ctypes.data_as(_c_int32_p)
    up = lambda a: a.ctypes.data_as(_c_uint8_p)
    pme = psd = None
    v = None
    if fund_options is not None:
        if pair_max_error is not None:
            pme = np.ascontiguousarray(pair_max_error, np.float64)
            if pme.shape != (npair,):
                raise ValueError("frames_match: pair_max_error must have one entry per pair")
        if pair_seed is not None:
            psd = np.ascontiguousarray(pair_seed, np.uint32)
            if psd.shape != (npair,):
                raise ValueError("frames_match: pair_seed must have one entry per pair")
        v = dict(status=np.zeros(npair, np.uint8), F=np.zeros((npair, 9)), inlier_mask=np.zeros(cap, np.uint8), num_inliers=np.zeros(npair, np.int32),
                 num_trials=np.zeros(npair, np.int32), best_trial=np.full(npair, -1, np.int32), accepted=np.zeros(npair, np.uint8))
    elif pair_max_error is not None or pair_seed is not None:
        raise ValueError("frames_match: pair_max_error and pair_seed belong to the verification (fund_options)")
    check(load().xrsfm_ba_frames_match(frames._h(), C.byref(mo), C.byref(fund_options) if v is not None else None, npair, ip(pair_a), ip(pair_b),
                                       _dp(pme), psd.ctypes.data_as(C.POINTER(C.c_uint32)) if psd is not None else None, cap,
                                       mp.ctypes.data_as(C.POINTER(C.c_int64)), ip(m), ip(r["num_row"]), ip(r["num_col"]),
                                       up(v["status"]) if v else None, _dp(v["F"]) if v else None, up(v["inlier_mask"]) if v else None,
                                       ip(v["num_inliers"]) if v else None, ip(v["num_trials"]) if v else None, ip(v["best_trial"]) if v else None,
                                       up(v["accepted"]) if v else None), "xrsfm_ba_frames_match")
    r["match_ptr"] = mp
    r["matches"] = m[:int(mp[-1])].copy()
    if v:
        v["inlier_mask"] = v["inlier_mask"][:int(mp[-1])].copy()
        r.update(v)
    return r


def expand_options(**overrides) -> CExpandOptions:
    """xrsfm_ba_expand_options_default: the constants of the reference's MatchExpansionSolver."""
    o = CExpandOptions()
    load().xrsfm_ba_expand_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


EXPAND_STATS = ("rounds", "tracks", "valid_tracks", "corr_entries", "items_walked", "codes_kept", "passes")


class _ExpandArgs:
    """the arrays the expansion entries share, kept alive for the call"""

    def __init__(self, name, n_frames, pair_a, pair_b, match_ptr, matches, sizes=None, rank_ptr=None, rank_ids=None, tried=None):
        i32 = lambda a: np.ascontiguousarray(a, np.int32)
        self.n = int(n_frames)
        self.pa, self.pb = i32(pair_a).reshape(-1), i32(pair_b).reshape(-1)
        self.mp = np.ascontiguousarray(match_ptr, np.int64).reshape(-1) if len(self.pa) else np.zeros(1, np.int64)
        self.m = i32(matches).reshape(-1, 2)
        if self.pa.shape != self.pb.shape or len(self.mp) != len(self.pa) + 1 or self.mp[-1] != len(self.m):
            raise ValueError(name + ": inconsistent pair and match arrays")
        if sizes is not None:
            sizes = i32(sizes).reshape(-1, 2)
            if len(sizes) != self.n:
                raise ValueError(name + ": one (width, height) per frame")
            self.w, self.h = np.ascontiguousarray(sizes[:, 0]), np.ascontiguousarray(sizes[:, 1])
        if rank_ptr is not None:
            self.rp = np.ascontiguousarray(rank_ptr, np.int64).reshape(-1)
            self.ri = i32(rank_ids).reshape(-1)
            if len(self.rp) != self.n + 1 or self.rp[-1] != len(self.ri):
                raise ValueError(name + ": inconsistent rank arrays")
            t = i32(tried if tried is not None else np.zeros((0, 2))).reshape(-1, 2)
            self.ta, self.tb = np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, 1])

    @staticmethod
    def ip(a):
        return a.ctypes.data_as(_c_int32_p)

    @staticmethod
    def lp(a):
        return a.ctypes.data_as(C.POINTER(C.c_int64))

    def pairs(self):
        return [len(self.pa), self.ip(self.pa), self.ip(self.pb), self.lp(self.mp), self.ip(self.m)]


def _expand_call(name, head, a: _ExpandArgs, init_a, init_b, with_cand):
    n, cap = a.n, len(a.ri)
    r = dict(connected=np.zeros(n, np.uint8), registered=np.zeros(n, np.uint8), may_register=np.zeros(n, np.uint8), visible=np.zeros(n, np.int32))
    oa, ob, src = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.uint8)
    cand = np.zeros((cap, 4), np.int32)
    n_out, n_cand = C.c_int64(0), C.c_int64(0)
    stats = np.zeros(8, np.int64)
    up = lambda x: x.ctypes.data_as(_c_uint8_p)
    check(getattr(load(), name)(*head, *a.pairs(), a.lp(a.rp), a.ip(a.ri), len(a.ta), a.ip(a.ta), a.ip(a.tb), int(init_a), int(init_b), cap, C.byref(n_out), a.ip(oa),
                                a.ip(ob), up(src), up(r["connected"]), up(r["registered"]), up(r["may_register"]), a.ip(r["visible"]), cap if with_cand else 0,
                                C.byref(n_cand) if with_cand else None, a.ip(cand) if with_cand else None, a.lp(stats)), name)
    k = int(n_out.value)
    r.update(pair_a=oa[:k].copy(), pair_b=ob[:k].copy(), source=src[:k].copy(), stats=dict(zip(EXPAND_STATS, (int(x) for x in stats))))
    if with_cand:
        r["cand"] = cand[:int(n_cand.value)].copy()
    return r


def expand_candidates(key_ptr, keys, sizes, pair_a, pair_b, match_ptr, matches, rank_ptr, rank_ids, init_a, init_b, tried=None,
                      options: CExpandOptions | None = None, with_cand: bool = True) -> dict:
    """xrsfm_ba_expand_candidates: one MatchExpansionSolver::Run.  keys [N][4] or [N][2] float32, sizes [n][2] (width, height), the
    verified pairs with their inlier matches (verified_matches), the retrieval lists as a CSR, tried [k][2].  Returns pair_a, pair_b,
    source (1 covisibility, 2 similarity), connected, registered, may_register, visible, cand [k][4] and stats."""
    o = options if options is not None else expand_options()
    key_ptr = np.ascontiguousarray(key_ptr, np.int64).reshape(-1)
    k = np.asarray(keys, np.float32).reshape(len(keys), -1) if len(keys) else np.zeros((0, 4), np.float32)
    if k.shape[1] == 2:
        k = np.concatenate([k, np.zeros((len(k), 2), np.float32)], axis=1)
    k = np.ascontiguousarray(k, np.float32)
    if k.shape[1] != 4 or key_ptr[-1] != len(k):
        raise ValueError("expand_candidates: inconsistent key arrays")
    a = _ExpandArgs("expand_candidates", len(key_ptr) - 1, pair_a, pair_b, match_ptr, matches, sizes, rank_ptr, rank_ids, tried)
    head = [C.byref(o), a.n, a.lp(key_ptr), k.ctypes.data_as(C.POINTER(C.c_float)), a.ip(a.w), a.ip(a.h)]
    return _expand_call("xrsfm_ba_expand_candidates", head, a, init_a, init_b, with_cand)


def frames_expand(frames: Frames, sizes, pair_a, pair_b, match_ptr, matches, rank_ptr, rank_ids, init_a, init_b, tried=None,
                  options: CExpandOptions | None = None, with_cand: bool = True) -> dict:
    """xrsfm_ba_frames_expand: expand_candidates on a resident set; no key point is uploaded."""
    o = options if options is not None else expand_options()
    a = _ExpandArgs("frames_expand", frames_info(frames)["n_frames"], pair_a, pair_b, match_ptr, matches, sizes, rank_ptr, rank_ids, tried)
    return _expand_call("xrsfm_ba_frames_expand", [frames._h(), C.byref(o), a.ip(a.w), a.ip(a.h)], a, init_a, init_b, with_cand)


def debug_expand_tracks(key_ptr, pair_a, pair_b, match_ptr, matches) -> dict:
    """xrsfm_ba_debug_expand_tracks (no GPU): key_track [N], track_ptr [T + 1], obs_frame, obs_key, invalid [T]."""
    key_ptr = np.ascontiguousarray(key_ptr, np.int64).reshape(-1)
    a = _ExpandArgs("debug_expand_tracks", len(key_ptr) - 1, pair_a, pair_b, match_ptr, matches)
    M = len(a.m)
    kt = np.zeros(max(int(key_ptr[-1]), 1), np.int32); tp = np.zeros(M + 1, np.int64); inv = np.zeros(max(M, 1), np.uint8)
    of, ok = np.zeros(max(2 * M, 1), np.int32), np.zeros(max(2 * M, 1), np.int32)
    nt, no = C.c_int64(0), C.c_int64(0)
    check(load().xrsfm_ba_debug_expand_tracks(a.n, a.lp(key_ptr), *a.pairs(), a.ip(kt), M, C.byref(nt), a.lp(tp), inv.ctypes.data_as(_c_uint8_p), 2 * M, C.byref(no),
                                              a.ip(of), a.ip(ok)), "xrsfm_ba_debug_expand_tracks")
    T, O = int(nt.value), int(no.value)
    return dict(key_track=kt[:int(key_ptr[-1])].copy(), track_ptr=tp[:T + 1].copy(), obs_frame=of[:O].copy(), obs_key=ok[:O].copy(), invalid=inv[:T].copy())


def debug_expand_covis(key_ptr, keys, sizes, pair_a, pair_b, match_ptr, matches, init_a, init_b, options: CExpandOptions | None = None) -> tuple:
    """xrsfm_ba_debug_expand_covis: (code_ptr [n + 1], codes) of k_expand_covis."""
    o = options if options is not None else expand_options()
    key_ptr = np.ascontiguousarray(key_ptr, np.int64).reshape(-1)
    k = np.ascontiguousarray(np.asarray(keys, np.float32).reshape(-1, 4))
    a = _ExpandArgs("debug_expand_covis", len(key_ptr) - 1, pair_a, pair_b, match_ptr, matches, sizes)
    cap = 2 * len(a.m) * max(a.n, 1)                  # (every observation of a track can be walked from each of its frames)
    cp = np.zeros(a.n + 1, np.int64); codes = np.zeros(max(cap, 1), np.int32)
    check(load().xrsfm_ba_debug_expand_covis(C.byref(o), a.n, a.lp(key_ptr), k.ctypes.data_as(C.POINTER(C.c_float)), a.ip(a.w), a.ip(a.h), *a.pairs(), int(init_a),
                                             int(init_b), cap, a.lp(cp), a.ip(codes)), "xrsfm_ba_debug_expand_covis")
    return cp, codes[:int(cp[-1])].copy()


def expansion_and_matching(frames: Frames, sizes, rank_ptr, rank_ids, init_pairs, init_a, init_b, num_iteration: int = 5,
                           options: CExpandOptions | None = None, match_options: CMatchOptions | None = None, fund_options: CFundOptions | None = None,
                           expand=None) -> dict:
    """The reference's ExpansionAndMatching (feature_processing.cc:324-377) on a resident set.  init_pairs [k][2]: the pairs of the
    first FeatureMatching (the retrieval's best); they are matched and verified first, then num_iteration times: expand, drop what was
    tried, frames_match, verified_matches, append the accepted pairs.  `expand` replaces frames_expand (a test passes its yardstick).
    Returns pair_a, pair_b, match_ptr, matches of the verified pairs in the order they were accepted, tried [k][2], and per iteration
    the counts the reference prints (candidates, accepted, pairs, matches)."""
    fo = fund_options if fund_options is not None else verify_pairs_options()
    expand = expand if expand is not None else frames_expand
    pa, pb, rows = [], [], []
    tried, seen, log = [], set(), []

    def match(a, b):
        r = frames_match(frames, a, b, match_options, fo)
        kept, m, _ = verified_matches(r, r["match_ptr"], r["matches"])
        mp = r["match_ptr"]
        mask = r["inlier_mask"].astype(bool)
        for p in kept:
            pa.append(int(a[p])); pb.append(int(b[p])); rows.append(r["matches"][mp[p]:mp[p + 1]][mask[mp[p]:mp[p + 1]]])
        for x, y in zip(a, b):
            tried.append((int(x), int(y))); seen.add((min(int(x), int(y)), max(int(x), int(y))))
        return len(kept)

    def state():
        ptr = np.zeros(len(rows) + 1, np.int64)
        if rows:
            ptr[1:] = np.cumsum([len(x) for x in rows])
        m = np.concatenate(rows).reshape(-1, 2) if rows else np.zeros((0, 2), np.int32)
        return np.array(pa, np.int32), np.array(pb, np.int32), ptr, np.ascontiguousarray(m, np.int32)

    ini = np.asarray(init_pairs, np.int32).reshape(-1, 2)
    accepted = match(ini[:, 0].copy(), ini[:, 1].copy())
    log.append(dict(candidates=len(ini), accepted=accepted, pairs=len(pa), matches=int(sum(len(x) for x in rows))))
    for _ in range(int(num_iteration)):
        a, b, ptr, m = state()
        r = expand(frames, sizes, a, b, ptr, m, rank_ptr, rank_ids, init_a, init_b, np.array(tried, np.int32).reshape(-1, 2), options)
        new = [(int(x), int(y)) for x, y in zip(r["pair_a"], r["pair_b"]) if (int(x), int(y)) not in seen]
        accepted = match(np.array([x for x, _ in new], np.int32), np.array([y for _, y in new], np.int32)) if new else 0
        log.append(dict(candidates=len(new), accepted=accepted, pairs=len(pa), matches=int(sum(len(x) for x in rows))))
    a, b, ptr, m = state()
    return dict(pair_a=a, pair_b=b, match_ptr=ptr, matches=m, tried=np.array(tried, np.int32).reshape(-1, 2), iterations=log)


def debug_sift_gradient(image, octave: int, options: CSiftOptions | None = None) -> np.ndarray:
    """xrsfm_ba_debug_sift_gradient: (grd, rot) of G[1..3] of one octave, [3][h][w][2]."""
    o = options if options is not None else sift_options()
    a = _grey(image)
    geo = sift_geometry(a.shape[1], a.shape[0], o)
    if not 0 <= octave < len(geo):
        raise ValueError("debug_sift_gradient: the image has no such octave")
    ws, hs = geo[octave]
    g = np.zeros((3, hs, ws, 2), np.float32)
    check(load().xrsfm_ba_debug_sift_gradient(C.byref(o), a.shape[1], a.shape[0], a.ctypes.data_as(_c_uint8_p), octave, g.ctypes.data_as(C.POINTER(C.c_float))),
          "xrsfm_ba_debug_sift_gradient")
    return g


def debug_sift_describe(image, options: CSiftOptions | None = None, desc_options: CSiftDescOptions | None = None) -> dict:
    """xrsfm_ba_debug_sift_describe: loc [n][4], okeys [n][4], raw [n][128], unit [n][128] of one image."""
    o = options if options is not None else sift_options()
    do = desc_options if desc_options is not None else sift_desc_options()
    a = _grey(image)
    n = C.c_int64(0)
    cap = 4096
    fp = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))
    for _ in range(2):
        l = np.zeros((cap, 4), np.int32); k = np.zeros((cap, 4), np.float32); r = np.zeros((cap, 128), np.float32); u = np.zeros((cap, 128), np.float32)
        code = load().xrsfm_ba_debug_sift_describe(C.byref(o), C.byref(do), a.shape[1], a.shape[0], a.ctypes.data_as(_c_uint8_p), cap, C.byref(n),
                                                   l.ctypes.data_as(_c_int32_p), fp(k), fp(r), fp(u))
        if code == EINVAL and n.value > cap:
            cap = int(n.value)
            continue
        break
    check(code, "xrsfm_ba_debug_sift_describe")
    m = n.value
    return dict(loc=l[:m].copy(), okeys=k[:m].copy(), raw=r[:m].copy(), unit=u[:m].copy())


# ---------------------------------------------------------------------------------------------------- track completion and merging
MERGE_CONTINUE, MERGE_MERGE, MERGE_FRAME = 1, 2, 4
MERGE_MAX_KEYS, MERGE_MAX_TRACKS = 1024, 512   # XRSFM_BA_MERGE_MAX_KEYS / _TRACKS: the largest component that is attempted
MERGE_STATS = ("merged", "connected_tracks", "continued", "connected_measurements", "components", "skipped", "largest")


def merge_options(**overrides) -> CMergeOptions:
    """xrsfm_ba_merge_options_default: 8.0 px, ContinueTrack then MergeTrack over every track (run_triangulation)."""
    o = CMergeOptions()
    load().xrsfm_ba_merge_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


class _MergeArgs:
    """the inputs the two merge entries share, kept alive for the call"""

    def __init__(self, name, key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key, points, track_outlier, track_of_key, options):
        c = np.ascontiguousarray
        self.o = options if options is not None else merge_options()
        self.key_ptr = c(key_ptr, np.int64).reshape(-1)
        self.n = len(self.key_ptr) - 1
        self.xy = c(key_xy, np.float64).reshape(-1, 2)
        self.reg, self.q, self.t = c(registered, np.uint8).reshape(-1), c(cam_q, np.float64).reshape(-1, 4), c(cam_t, np.float64).reshape(-1, 3)
        self.ci, self.im, self.ip = c(cam_intr, np.int32).reshape(-1), c(intr_model, np.int32).reshape(-1), c(intr_params, np.float64).reshape(-1, 8)
        self.cp = c(corr_ptr, np.int64).reshape(-1) if len(self.xy) else np.zeros(1, np.int64)
        self.ck = c(corr_key, np.int32).reshape(-1)
        self.points = np.array(points, np.float64, order="C").reshape(-1, 3)             # copies: the call writes them
        self.outlier = np.array(track_outlier, np.uint8).reshape(-1)
        self.tok = np.array(track_of_key, np.int32).reshape(-1)
        N = len(self.xy)
        if self.n < 0 or len(self.reg) != self.n or len(self.q) != self.n or len(self.t) != self.n or len(self.ci) != self.n or len(self.im) != len(self.ip) or \
                len(self.tok) != N or len(self.cp) != N + 1 or len(self.outlier) != len(self.points) or (N and (self.key_ptr[-1] != N or self.cp[-1] != len(self.ck))):
            raise ValueError(name + ": inconsistent array lengths")

    def head(self):
        lp, ip, up = (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))), (lambda a: a.ctypes.data_as(_c_int32_p)), (lambda a: a.ctypes.data_as(_c_uint8_p))
        return [C.byref(self.o), self.n, lp(self.key_ptr), _dp(self.xy), up(self.reg), _dp(self.q), _dp(self.t), ip(self.ci), len(self.im), ip(self.im), _dp(self.ip),
                lp(self.cp), ip(self.ck), len(self.points), _dp(self.points), up(self.outlier), ip(self.tok)]


def merge_tracks(key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key, points, track_outlier, track_of_key,
                 options: CMergeOptions | None = None) -> dict:
    """xrsfm_ba_merge_tracks: ContinueTrack / MergeTrack over every track, or MergeTracks(frame), by options.mode.  The three state
    arrays are not changed; the result holds their new values (points, track_outlier, track_of_key) and track_status,
    corr_have_point3d [N], visible and measured [n_frames], stats."""
    a = _MergeArgs("merge_tracks", key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key, points, track_outlier, track_of_key,
                   options)
    status, have = np.zeros(len(a.points), np.uint8), np.zeros(len(a.tok), np.int32)
    vis, mea, stats = np.zeros(a.n, np.int32), np.zeros(a.n, np.int32), np.zeros(8, np.int64)
    ip = lambda x: x.ctypes.data_as(_c_int32_p)
    check(load().xrsfm_ba_merge_tracks(*a.head(), status.ctypes.data_as(_c_uint8_p), ip(have), ip(vis), ip(mea), stats.ctypes.data_as(C.POINTER(C.c_int64))),
          "xrsfm_ba_merge_tracks")
    return dict(points=a.points, track_outlier=a.outlier, track_of_key=a.tok, track_status=status, corr_have_point3d=have, visible=vis, measured=mea,
                stats=dict(zip(MERGE_STATS, (int(x) for x in stats))))


def debug_merge_components(key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key, points, track_outlier, track_of_key,
                           options: CMergeOptions | None = None) -> tuple:
    """xrsfm_ba_debug_merge_components (no GPU): (comp_of_key [N], number of components), largest component first."""
    a = _MergeArgs("debug_merge_components", key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, intr_model, intr_params, corr_ptr, corr_key, points, track_outlier,
                   track_of_key, options)
    comp, n = np.zeros(len(a.tok), np.int32), C.c_int32(0)
    check(load().xrsfm_ba_debug_merge_components(*a.head(), comp.ctypes.data_as(_c_int32_p), C.byref(n)), "xrsfm_ba_debug_merge_components")
    return comp, int(n.value)


def _csr_entries(ptr, rows):
    """the entries ptr[r] .. ptr[r + 1] of every row in rows, behind one another"""
    cnt = ptr[rows + 1] - ptr[rows]
    if cnt.sum() == 0:
        return np.zeros(0, np.int64)
    return np.repeat(ptr[rows] - np.concatenate([[0], np.cumsum(cnt)[:-1]]), cnt) + np.arange(cnt.sum())


def correspondence_graph(key_ptr, pair_a, pair_b, match_ptr, matches) -> tuple:
    """The lists of Map::Init (src/base/map.cc:55-83) as a CSR over global key indices, in its insertion order: pairs in list order,
    a pair's matches in order, each match appended to both key points' lists.  matches [M][2]: the inliers alone.  -> (corr_ptr, corr_key)"""
    key_ptr = np.asarray(key_ptr, np.int64).reshape(-1)
    pa, pb = np.asarray(pair_a, np.int64).reshape(-1), np.asarray(pair_b, np.int64).reshape(-1)
    mp, m = np.asarray(match_ptr, np.int64).reshape(-1), np.asarray(matches, np.int64).reshape(-1, 2)
    N = int(key_ptr[-1])
    pair_of = np.repeat(np.arange(len(pa)), np.diff(mp)) if len(pa) else np.zeros(0, np.int64)
    ka, kb = key_ptr[pa[pair_of]] + m[:, 0], key_ptr[pb[pair_of]] + m[:, 1]
    src, dst = np.stack([ka, kb], axis=1).reshape(-1), np.stack([kb, ka], axis=1).reshape(-1)
    order = np.argsort(src, kind="stable")
    ptr = np.zeros(N + 1, np.int64)
    np.cumsum(np.bincount(src, minlength=N), out=ptr[1:])
    return ptr, dst[order].astype(np.int32)


def merge_closure(frame: int, key_ptr, corr_ptr, corr_key, track_of_key) -> dict:
    """The sub-map made of the whole components (key points; edges: list entries and "same track") that hold a key point of `frame`
    with a track: what xrsfm_ba_merge_tracks processes in frame mode on that frame.  -> keys (the global key indices, ascending),
    tracks (the global track ids, ascending), and the sub-map's key_ptr (every frame kept), corr_ptr, corr_key and track_of_key in
    its own indices.  A caller gathers key_xy[keys], points[tracks] and track_outlier[tracks], calls merge_tracks, and scatters
    track_of_key (through tracks), points and outliers back."""
    key_ptr, cp = np.asarray(key_ptr, np.int64).reshape(-1), np.asarray(corr_ptr, np.int64).reshape(-1)
    ck, tok = np.asarray(corr_key, np.int64).reshape(-1), np.asarray(track_of_key, np.int64).reshape(-1)
    N = len(tok)
    inside, track_in = np.zeros(N, bool), np.zeros(int(tok.max()) + 2 if N else 1, bool)
    front = np.arange(key_ptr[frame], key_ptr[frame + 1])
    front = front[tok[front] >= 0]
    while len(front):
        inside[front] = True
        t = np.unique(tok[front][tok[front] >= 0])
        t = t[~track_in[t]]
        track_in[t] = True
        same = np.nonzero(np.isin(tok, t))[0] if len(t) else np.zeros(0, np.int64)
        front = np.unique(np.concatenate([ck[_csr_entries(cp, front)], same]))
        front = front[~inside[front]]
    keys = np.nonzero(inside)[0]
    local = np.full(N, -1, np.int64)
    local[keys] = np.arange(len(keys))
    tracks = np.nonzero(track_in)[0]
    tlocal = np.full(len(track_in), -1, np.int64)
    tlocal[tracks] = np.arange(len(tracks))
    sub_ptr = np.concatenate([[0], np.cumsum(cp[keys + 1] - cp[keys])]).astype(np.int64)
    sub_tok = np.where(tok[keys] >= 0, tlocal[np.maximum(tok[keys], 0)], -1).astype(np.int32)
    return dict(keys=keys, tracks=tracks, key_ptr=np.searchsorted(keys, key_ptr).astype(np.int64), corr_ptr=sub_ptr,
                corr_key=local[ck[_csr_entries(cp, keys)]].astype(np.int32), track_of_key=sub_tok)


TRIF_STATS = ("created", "zero_track", "extended", "one_track", "multi_track", "steps", "split_frames", "claim_rounds")


def trif_options(**overrides) -> CTrifOptions:
    """xrsfm_ba_trif_options_default: DegToRad(8.0) and the settings of CreatePoint3d1.  extend_angle_rad, or a field of the embedded
    CTriOptions by its name."""
    o = CTrifOptions()
    load().xrsfm_ba_trif_options_default(C.byref(o))
    for k, v in overrides.items():
        if k == "extend_angle_rad":
            o.extend_angle_rad = v
        elif hasattr(o.tri, k):
            setattr(o.tri, k, v)
        else:
            raise AttributeError(k)
    return o


def trif_capacity(key_ptr, registered, corr_ptr, corr_key, frames, n_tracks, track_of_key) -> int:
    """the bound xrsfm_ba_triangulate_frames asks of track_capacity: n_tracks plus the key points without a track of the listed
    frames that have an entry in a registered frame"""
    key_ptr, cp = np.asarray(key_ptr, np.int64).reshape(-1), np.asarray(corr_ptr, np.int64).reshape(-1)
    ck, tok, reg = np.asarray(corr_key, np.int64).reshape(-1), np.asarray(track_of_key).reshape(-1), np.asarray(registered).reshape(-1) != 0
    frame_of_key = np.repeat(np.arange(len(key_ptr) - 1), np.diff(key_ptr))
    entry_reg = reg[frame_of_key[ck]].astype(np.int64) if len(ck) else np.zeros(0, np.int64)
    has = np.diff(np.concatenate([[0], np.cumsum(entry_reg)])[cp]) > 0 if len(tok) else np.zeros(0, bool)
    listed = np.zeros(len(key_ptr) - 1, bool)
    listed[np.asarray(frames, np.int64).reshape(-1)] = True
    return int(n_tracks) + int((listed[frame_of_key] & (tok == -1) & has).sum())


def triangulate_frames(key_ptr, key_xyn, registered, cam_q, cam_t, corr_ptr, corr_key, frames, points, track_outlier, track_of_key,
                       options: CTrifOptions | None = None, capacity: int | None = None) -> dict:
    """xrsfm_ba_triangulate_frames: TriangulateFramePoint for the listed frames, one after another.  The three state arrays are not
    changed; the result holds their new values (points and track_outlier cut to n_tracks), key_status and the create diagnostics
    [N], corr_have_point3d [N], visible and measured [n_frames], stats.  The capacity is the call's bound unless given."""
    c = np.ascontiguousarray
    o = options if options is not None else trif_options()
    key_ptr = c(key_ptr, np.int64).reshape(-1)
    n = len(key_ptr) - 1
    xy = c(key_xyn, np.float64).reshape(-1, 2)
    N = len(xy)
    reg, q, t = c(registered, np.uint8).reshape(-1), c(cam_q, np.float64).reshape(-1, 4), c(cam_t, np.float64).reshape(-1, 3)
    cp = c(corr_ptr, np.int64).reshape(-1) if N else np.zeros(1, np.int64)
    ck = c(corr_key, np.int32).reshape(-1)
    frames = c(frames, np.int32).reshape(-1)
    p0, out0, tok = c(points, np.float64).reshape(-1, 3), c(track_outlier, np.uint8).reshape(-1), np.array(track_of_key, np.int32).reshape(-1)
    T = len(p0)
    if n < 0 or len(reg) != n or len(q) != n or len(t) != n or len(tok) != N or len(cp) != N + 1 or len(out0) != T or (N and (key_ptr[-1] != N or cp[-1] != len(ck))):
        raise ValueError("triangulate_frames: inconsistent array lengths")
    if capacity is None:
        ok = len(frames) == 0 or (frames.min() >= 0 and frames.max() < n)
        capacity = trif_capacity(key_ptr, reg, cp, ck, frames, T, tok) if ok and N else T        # (a bad list is the call's to refuse)
    cap = max(int(capacity), 0)
    pts, outl = np.zeros((max(cap, T), 3)), np.zeros(max(cap, T), np.uint8)
    pts[:T] = p0; outl[:T] = out0
    status, ninl, ntr, best = np.zeros(N, np.uint8), np.zeros(N, np.int32), np.zeros(N, np.int32), np.full(N, -1, np.int32)
    have, vis, mea, stats, nout = np.zeros(N, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(8, np.int64), C.c_int32(T)
    ip, up, lp = (lambda a: a.ctypes.data_as(_c_int32_p)), (lambda a: a.ctypes.data_as(_c_uint8_p)), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int64)))
    check(load().xrsfm_ba_triangulate_frames(C.byref(o), n, lp(key_ptr), _dp(xy), up(reg), _dp(q), _dp(t), lp(cp), ip(ck), len(frames), ip(frames), T, int(capacity), _dp(pts),
                                             up(outl), ip(tok), C.byref(nout), up(status), ip(ninl), ip(ntr), ip(best), ip(have), ip(vis), ip(mea), lp(stats)),
          "xrsfm_ba_triangulate_frames")
    T1 = int(nout.value)
    return dict(points=pts[:T1].copy(), track_outlier=outl[:T1].copy(), track_of_key=tok, n_tracks=T1, key_status=status, num_inliers=ninl, num_trials=ntr,
                best_trial=best, corr_have_point3d=have, visible=vis, measured=mea, stats=dict(zip(TRIF_STATS, (int(x) for x in stats))))
