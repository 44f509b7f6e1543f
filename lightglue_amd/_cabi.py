"""ctypes binding of the C ABI declared in ``include/lightglue_amd.h``.

The shared library ``liblightglue_amd.so`` is built in-tree by ``lightglue_amd/csrc/Makefile``
(``__graft_entry__.build()``).  There is NO fallback: if the library is missing or fails to load,
``load()`` raises, and so does every product entry point that needs it.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

# LIGHTGLUE_AMD_LIB overrides the library file (A/B timing of two builds in one process tree); it must still be
# a build of this package's csrc/ — there is no other implementation to fall back to.
_LIB_PATH = Path(os.environ.get("LIGHTGLUE_AMD_LIB") or Path(__file__).resolve().parent / "liblightglue_amd.so")

LG_PREC = {"fp32": 0, "bf16": 1, "fp16": 2, "f16x3": 4}   # include/lightglue_amd.h LG_PREC_* (3 was split-bf16, removed in round 3)
LG_OK, LG_ERR_INVALID, LG_ERR_HIP, LG_ERR_STATE, LG_ERR_RANGE, LG_ERR_DEVICE, LG_ERR_INDEX = 0, 1, 2, 3, 4, 5, 6
LG_ERR_CAMERA = 7                                 # lg_relpose_estimate's per-pair status: a focal length that is not finite and > 0, or a non-finite principal point
LG_FLAG_NO_PRUNING, LG_FLAG_EXT, LG_FLAG_CHECK_FINITE, LG_FLAG_INDEXED = 1, 2, 4, 8
LG_FLAG_DESC0_F16, LG_FLAG_DESC1_F16 = 16, 32   # desc0 / desc1 are binary16 rows, read in place
LG_FLAG_DESC0_U8, LG_FLAG_DESC1_U8 = 64, 128    # desc0 / desc1 are uint8 rows (SIFT as COLMAP / OpenCV store it), read in place
LG_FLAG_ROOTSIFT0, LG_FLAG_ROOTSIFT1 = 256, 512   # RootSIFT of every row of desc0 / desc1 where the descriptors enter the engine
LG_DESC_KIND = {"float32": 0, "float16": 1, "uint8": 2}   # lg_rootsift src_kind
LG_FLAG_NN_MUTUAL = 1024                          # lg_nn_match: keep a match only if both directions agree
LG_EXTRACT_RAGGED, LG_EXTRACT_DESC_F16, LG_EXTRACT_SPLIT = 1, 2, 4   # the extractor stages' io flags: `sizes` is read / binary16 descriptors / split-f16 SuperPoint conv stack
LG_TWOVIEW_HOMOGRAPHY, LG_TWOVIEW_FUNDAMENTAL, LG_TWOVIEW_REFINE, LG_TWOVIEW_GIVEN_MODELS = 2048, 4096, 8192, 16384   # lg_twoview_verify's io flags
LG_RELPOSE_REFINE, LG_RELPOSE_ROOTS = 32768, 10   # lg_relpose_estimate: its refit flag, candidate models per hypothesis
LG_ABSPOSE_REFINE, LG_ABSPOSE_GROUPED, LG_ABSPOSE_GIVEN_POSES, LG_ABSPOSE_ROOTS = 65536, 131072, 262144, 4   # lg_abspose_estimate: its io flags, candidates per hypothesis
LG_TRI_REFINE, LG_TRI_TRACKS_ONLY, LG_TRI_MAX_TRACK_LENGTH = 524288, 1048576, 1024   # lg_triangulate: its io flags, the longest track it triangulates
LG_TRI_MAX_HYPOTHESES, LG_TRI_MAX_TRACKS = 4096, 4   # lg_triangulate_robust: hypotheses per round, rounds (tracks) per component
LG_BA_MAX_IMAGES, LG_BA_MAX_ITERATIONS, LG_BA_MAX_TRACK_LENGTH, LG_BA_CHOLESKY_BLOCK = 256, 100, 1024, 48   # lg_bundle_adjust: its envelope, the columns per Cholesky panel (it defines no flag bit)
LG_BA_LOSS = {"squared": 0, "huber": 1, "cauchy": 2}   # lg_bundle_adjust_robust: LG_BA_LOSS_*
LG_BA_MAX_FILTER_ROUNDS = 4                         # lg_bundle_adjust_robust: filters (stages - 1) of one call
LG_BA_PCG_MAX_IMAGES, LG_BA_PCG_MAX_CG_ITERATIONS, LG_BA_PCG_MAX_SOLVER_ITERATIONS = 4096, 1000, 20000   # lg_bundle_adjust_pcg: its envelope (solver iterations: enqueued per call)
LG_PG_MIN_ITERATIONS, LG_PG_MAX_PAIRS = 6, 2 ** 20   # lg_posegraph_solve: its envelope next to LG_BA_MAX_IMAGES and LG_BA_MAX_ITERATIONS (it defines no flag bit)
LG_TWOVIEW_TILE = 256                             # lg_twoview_verify: correspondences per LDS tile of the scoring kernel (= hypotheses per workgroup)
LG_NN_ROWS_PER_WORKGROUP, LG_NN_TILE = 128, 64    # lg_nn_match's kernel shape: rows of one side a workgroup owns, rows of the other side per LDS tile
LG_MAX_KEYPOINTS, LG_MAX_ROWS, LG_MAX_SIM_ELEMS = 8192, 2 ** 21, 2 ** 31 - 1   # the envelope of one lg_engine_forward call

# every symbol include/lightglue_amd.h declares (tests check the library exports all of them)
EXPORTED_SYMBOLS = (
    "lg_last_error", "lg_version", "lg_engine_create", "lg_engine_destroy", "lg_engine_set_weight",
    "lg_engine_finalize_weights", "lg_engine_reserve", "lg_engine_forward", "lg_unpack_wire", "lg_engine_set_option",
    "lg_engine_debug_stop_after", "lg_engine_debug_read", "lg_engine_debug_caps",
    "lg_profile_num_classes", "lg_profile_class_name", "lg_engine_profile_enable", "lg_engine_profile_read",
    "lg_sp_sample_descriptors", "lg_sp_detect_workspace_bytes", "lg_sp_detect",
    "lg_sp_pack_conv_weight", "lg_sp_encode_workspace_bytes", "lg_sp_encode", "lg_sp_pack_conv_weight_split", "lg_debug_mfma_sustained",
    "lg_aliked_packed_bytes", "lg_aliked_pack_weights", "lg_aliked_levels_bytes", "lg_aliked_workspace_bytes", "lg_aliked_encode",
    "lg_aliked_detect_workspace_bytes", "lg_aliked_detect", "lg_aliked_describe_workspace_bytes", "lg_aliked_describe",
    "lg_preprocess_plan", "lg_preprocess_resize",
    "lg_preprocess_ragged_table_bytes", "lg_preprocess_ragged_plan", "lg_preprocess_resize_ragged",
    "lg_rootsift", "lg_sift_filter_workspace_bytes", "lg_sift_filter",
    "lg_nn_workspace_bytes", "lg_nn_match",
    "lg_twoview_workspace_bytes", "lg_twoview_verify",
    "lg_relpose_workspace_bytes", "lg_relpose_estimate",
    "lg_abspose_workspace_bytes", "lg_abspose_estimate",
    "lg_triangulate_workspace_bytes", "lg_triangulate", "lg_triangulate_robust_workspace_bytes", "lg_triangulate_robust",
    "lg_bundle_workspace_bytes", "lg_bundle_adjust", "lg_bundle_robust_workspace_bytes", "lg_bundle_adjust_robust", "lg_bundle_focal_workspace_bytes", "lg_bundle_adjust_focal",
    "lg_bundle_pcg_workspace_bytes", "lg_bundle_adjust_pcg",
    "lg_posegraph_workspace_bytes", "lg_posegraph_solve",
    "lg_posegraph_pcg_workspace_bytes", "lg_posegraph_solve_pcg",
    "lg_positioning_workspace_bytes", "lg_positioning_solve",
)


class LgConfig(C.Structure):
    _fields_ = [
        ("input_dim", C.c_int32), ("descriptor_dim", C.c_int32), ("n_layers", C.c_int32), ("num_heads", C.c_int32),
        ("add_scale_ori", C.c_int32),
        ("depth_confidence", C.c_double), ("width_confidence", C.c_double), ("filter_threshold", C.c_double),
        ("pruning_min_kpts", C.c_int32), ("precision", C.c_int32), ("attn_precision", C.c_int32),
    ]


_fp = C.c_void_p  # device pointers travel as integers


class LgForwardIO(C.Structure):
    _fields_ = [
        ("batch", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32), ("flags", C.c_uint32),
        ("kpts0", _fp), ("kpts1", _fp), ("desc0", _fp), ("desc1", _fp), ("size0", _fp), ("size1", _fp),
        ("scales0", _fp), ("oris0", _fp), ("scales1", _fp), ("oris1", _fp),
        ("matches0", _fp), ("matches1", _fp), ("scores0", _fp), ("scores1", _fp), ("stop", _fp),
        ("prune0", _fp), ("prune1", _fp), ("matches", _fp), ("match_scores", _fp), ("n_matches", _fp),
        ("num0", _fp), ("num1", _fp), ("log_assignment", _fp),
        # round-5 extension (read by the engine only when flags & LG_FLAG_EXT)
        ("matches0_i64", _fp), ("matches1_i64", _fp), ("matches_i64", _fp), ("stop_i64", _fp),
        ("prune0_i64", _fp), ("prune1_i64", _fp), ("prune0_f32", _fp), ("prune1_f32", _fp),
        ("wire", _fp), ("wire_stride", C.c_int64), ("status", _fp),
        # indexed inputs (read only when flags & LG_FLAG_INDEXED)
        ("index0", _fp), ("index1", _fp), ("images0", C.c_int32), ("images1", C.c_int32),
    ]


class LgUnpackIO(C.Structure):
    """lg_unpack_io (include/lightglue_amd.h): the receiving side of the pair-sharded wire row"""
    _fields_ = [
        ("wire", _fp), ("wire_stride", C.c_int64), ("rows", C.c_int32),
        ("n0", C.c_int32), ("n1", C.c_int32), ("with_prune", C.c_int32), ("pairs_out", C.c_int32),
        ("order", _fp),
        ("matches0", _fp), ("matches1", _fp), ("stop", _fp),
        ("scores0", _fp), ("scores1", _fp),
        ("prune0_i64", _fp), ("prune1_i64", _fp), ("prune0_f32", _fp), ("prune1_f32", _fp),
        ("matches", _fp), ("match_scores", _fp),
        ("info", _fp),
    ]


class LgNnIO(C.Structure):
    """lg_nn_io (include/lightglue_amd.h): one call of the nearest-neighbour matcher"""
    _fields_ = [
        ("pairs", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32), ("dim", C.c_int32), ("flags", C.c_uint32),
        ("ratio_threshold", C.c_float), ("distance_threshold", C.c_float),
        ("desc0", _fp), ("desc1", _fp), ("num0", _fp), ("num1", _fp), ("index0", _fp), ("index1", _fp), ("images0", C.c_int32), ("images1", C.c_int32),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("raw0", _fp), ("raw1", _fp), ("matches0", _fp), ("matches1", _fp), ("scores0", _fp), ("scores1", _fp),
        ("matches", _fp), ("match_scores", _fp), ("list_rows", C.c_int32), ("n_matches", _fp), ("status", _fp),
        ("stop", _fp), ("stop_i64", _fp), ("prune0", _fp), ("prune1", _fp),
    ]


class LgTwoViewIO(C.Structure):
    """lg_twoview_io (include/lightglue_amd.h): one call of the two-view verifier"""
    _fields_ = [
        ("pairs", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32), ("images0", C.c_int32), ("images1", C.c_int32), ("flags", C.c_uint32),
        ("threshold", C.c_float), ("num_hypotheses", C.c_int32), ("seed", C.c_uint32),
        ("kpts0", _fp), ("kpts1", _fp), ("num0", _fp), ("num1", _fp), ("index0", _fp), ("index1", _fp), ("matches0", _fp), ("models_in", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("models", _fp), ("inliers0", _fp), ("num_inliers", _fp), ("matches0_out", _fp), ("best_hypothesis", _fp), ("status", _fp),
    ]


class LgRelPoseIO(C.Structure):
    """lg_relpose_io (include/lightglue_amd.h): one call of the relative-pose estimator"""
    _fields_ = [
        ("pairs", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32), ("images0", C.c_int32), ("images1", C.c_int32), ("flags", C.c_uint32),
        ("threshold", C.c_float), ("num_hypotheses", C.c_int32), ("seed", C.c_uint32),
        ("kpts0", _fp), ("kpts1", _fp), ("num0", _fp), ("num1", _fp), ("index0", _fp), ("index1", _fp), ("matches0", _fp), ("cameras0", _fp), ("cameras1", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("rotations", _fp), ("translations", _fp), ("essentials", _fp), ("models", _fp), ("candidates", _fp),
        ("inliers0", _fp), ("num_inliers", _fp), ("matches0_out", _fp), ("best_hypothesis", _fp), ("num_in_front", _fp), ("status", _fp),
    ]


class LgAbsposeIO(C.Structure):
    """lg_abspose_io (include/lightglue_amd.h): one call of the absolute-pose estimator"""
    _fields_ = [
        ("pairs", C.c_int32), ("n0", C.c_int32), ("n1", C.c_int32), ("images0", C.c_int32), ("images1", C.c_int32), ("groups", C.c_int32), ("flags", C.c_uint32),
        ("threshold", C.c_float), ("num_hypotheses", C.c_int32), ("seed", C.c_uint32),
        ("kpts0", _fp), ("points3d1", _fp), ("num0", _fp), ("num1", _fp), ("index0", _fp), ("index1", _fp), ("matches0", _fp), ("cameras0", _fp),
        ("group_offsets", _fp), ("group_pairs", _fp), ("poses_in", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("rotations", _fp), ("translations", _fp), ("num_inliers", _fp), ("best_hypothesis", _fp), ("candidates", _fp),
        ("inliers0", _fp), ("pair_num_inliers", _fp), ("matches0_out", _fp), ("status", _fp),
    ]


class LgTriangulateIO(C.Structure):
    """lg_triangulate_io (include/lightglue_amd.h): one call of the triangulator"""
    _fields_ = [
        ("pairs", C.c_int32), ("n", C.c_int32), ("images", C.c_int32), ("flags", C.c_uint32),
        ("max_reproj_error", C.c_float), ("min_angle", C.c_float), ("max_track_length", C.c_int32),
        ("kpts", _fp), ("num", _fp), ("index0", _fp), ("index1", _fp), ("matches0", _fp), ("cameras", _fp), ("poses", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("points3d", _fp), ("track_id", _fp), ("node_state", _fp), ("xyz", _fp), ("track_length", _fp), ("track_error", _fp), ("counts", _fp), ("status", _fp),
    ]


class LgTriangulateRobustIO(C.Structure):
    """lg_triangulate_robust_io (include/lightglue_amd.h): one call of the triangulator's robust mode"""
    _fields_ = [("base", LgTriangulateIO), ("num_hypotheses", C.c_int32), ("max_tracks", C.c_int32), ("outlier_counts", _fp)]


class LgBundleIO(C.Structure):
    """lg_bundle_io (include/lightglue_amd.h): one call of the bundle adjuster"""
    _fields_ = [
        ("n", C.c_int32), ("images", C.c_int32), ("tracks", C.c_int32), ("flags", C.c_uint32), ("num_iterations", C.c_int32),
        ("initial_damping", C.c_double), ("function_tolerance", C.c_double),
        ("kpts", _fp), ("num", _fp), ("track_id", _fp), ("xyz", _fp), ("cameras", _fp), ("poses", _fp), ("constant_pose", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("poses_out", _fp), ("xyz_out", _fp), ("points3d", _fp), ("node_state", _fp), ("observation_error", _fp), ("summary", _fp), ("status", _fp),
    ]


class LgBundleRobustIO(C.Structure):
    """lg_bundle_robust_io (include/lightglue_amd.h): one call of the bundle adjuster's robust mode"""
    _fields_ = [("base", LgBundleIO), ("loss", C.c_int32), ("filter_rounds", C.c_int32), ("loss_scale", C.c_double), ("max_reproj_error", C.c_double)]


class LgBundleFocalIO(C.Structure):
    """lg_bundle_focal_io (include/lightglue_amd.h): one call of the bundle adjuster with per-image focal lengths refined"""
    _fields_ = [("base", LgBundleRobustIO), ("constant_camera", _fp), ("cameras_out", _fp)]


class LgBundlePcgIO(C.Structure):
    """lg_bundle_pcg_io (include/lightglue_amd.h): one call of the bundle adjuster with the iterative solver"""
    _fields_ = [("base", LgBundleRobustIO), ("max_cg_iterations", C.c_int32), ("pad", C.c_int32), ("cg_tolerance", C.c_double)]


class LgPosegraphIO(C.Structure):
    """lg_posegraph_io (include/lightglue_amd.h): one call of the global pose estimator"""
    _fields_ = [
        ("images", C.c_int32), ("pairs", C.c_int32), ("flags", C.c_uint32), ("num_iterations", C.c_int32), ("origin", C.c_int32), ("baseline", C.c_int32),
        ("min_inliers", C.c_int32), ("rotation_scale", C.c_double), ("max_rotation_error", C.c_double), ("direction_scale", C.c_double),
        ("pair_index", _fp), ("rotations", _fp), ("translations", _fp), ("weights", _fp), ("num_inliers", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("poses", _fp), ("image_state", _fp), ("pair_state", _fp), ("rotation_error", _fp), ("direction_error", _fp), ("summary", _fp),
    ]


class LgPosegraphPcgIO(C.Structure):
    """lg_posegraph_pcg_io (include/lightglue_amd.h): one call of the global pose estimator with the iterative solver"""
    _fields_ = [("base", LgPosegraphIO), ("rotation_cg_iterations", C.c_int32), ("position_cg_iterations", C.c_int32), ("cg_tolerance", C.c_double)]


class LgPositioningIO(C.Structure):
    """lg_positioning_io (include/lightglue_amd.h): one call of the global positioner"""
    _fields_ = [
        ("n", C.c_int32), ("images", C.c_int32), ("tracks", C.c_int32), ("flags", C.c_uint32), ("num_iterations", C.c_int32),
        ("angle_scale", C.c_double), ("max_angle_error", C.c_double),
        ("kpts", _fp), ("num", _fp), ("track_id", _fp), ("cameras", _fp), ("poses", _fp), ("constant_pose", _fp),
        ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("poses_out", _fp), ("xyz", _fp), ("points3d", _fp), ("track_id_out", _fp), ("node_state", _fp), ("image_state", _fp), ("angle_error", _fp),
        ("summary", _fp), ("status", _fp),
    ]


# The io structs of the six extractor stages (include/lightglue_amd.h): the variants of a stage are bits of `flags` (LG_EXTRACT_*), `sizes` is read only with
# LG_EXTRACT_RAGGED.  tests/test_cabi_symbols.py checks field order AND element types against the header.
_i32 = C.c_int32


class LgSpSampleIO(C.Structure):
    """lg_sp_sample_io: lg_sp_sample_descriptors"""
    _fields_ = [
        ("batch", _i32), ("channels", _i32), ("h", _i32), ("w", _i32), ("flags", C.c_uint32),
        ("desc_map", _fp), ("sizes", _fp), ("keypoints", _fp), ("num", _fp),
        ("n", _i32), ("cell", _i32), ("normalize_dense", _i32), ("workspace", _fp), ("out", _fp),
    ]


class LgSpEncodeIO(C.Structure):
    """lg_sp_encode_io: lg_sp_encode; `params` is a host array of the 24 device pointers"""
    _fields_ = [
        ("batch", _i32), ("h", _i32), ("w", _i32), ("flags", C.c_uint32),
        ("image", _fp), ("sizes", _fp), ("params", C.POINTER(C.c_void_p)), ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("scores", _fp), ("desc_map", _fp),
    ]


class LgSpDetectIO(C.Structure):
    """lg_sp_detect_io: lg_sp_detect"""
    _fields_ = [
        ("batch", _i32), ("h", _i32), ("w", _i32), ("flags", C.c_uint32),
        ("scores", _fp), ("sizes", _fp), ("nms_radius", _i32), ("remove_borders", _i32), ("detection_threshold", C.c_float),
        ("max_keypoints", _i32), ("capacity", _i32), ("max_candidates", _i32), ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("keypoints", _fp), ("kp_scores", _fp), ("counts", _fp), ("totals", _fp),
    ]


class LgAlikedEncodeIO(C.Structure):
    """lg_aliked_encode_io: lg_aliked_encode"""
    _fields_ = [
        ("batch", _i32), ("channels", _i32), ("h", _i32), ("w", _i32), ("n_pos", _i32), ("flags", C.c_uint32),
        ("image", _fp), ("sizes", _fp), ("packed", _fp), ("levels", _fp), ("workspace", _fp), ("workspace_bytes", C.c_int64), ("scores", _fp),
    ]


class LgAlikedDetectIO(C.Structure):
    """lg_aliked_detect_io: lg_aliked_detect"""
    _fields_ = [
        ("batch", _i32), ("h", _i32), ("w", _i32), ("flags", C.c_uint32),
        ("scores", _fp), ("sizes", _fp), ("image_size", _fp), ("nms_radius", _i32), ("scores_th", C.c_float),
        ("top_k", _i32), ("n_limit", _i32), ("capacity", _i32), ("workspace", _fp), ("workspace_bytes", C.c_int64),
        ("keypoints", _fp), ("kp_scores", _fp), ("kp_norm", _fp), ("counts", _fp),
    ]


class LgAlikedDescribeIO(C.Structure):
    """lg_aliked_describe_io: lg_aliked_describe"""
    _fields_ = [
        ("batch", _i32), ("h", _i32), ("w", _i32), ("n_pos", _i32), ("flags", C.c_uint32),
        ("levels", _fp), ("sizes", _fp), ("packed", _fp), ("kp_norm", _fp), ("counts", _fp),
        ("n", _i32), ("workspace", _fp), ("workspace_bytes", C.c_int64), ("descriptors", _fp),
    ]


# entry point -> its io struct
EXTRACT_STAGES = {"lg_sp_encode": LgSpEncodeIO, "lg_sp_detect": LgSpDetectIO, "lg_sp_sample_descriptors": LgSpSampleIO,
                  "lg_aliked_encode": LgAlikedEncodeIO, "lg_aliked_detect": LgAlikedDetectIO, "lg_aliked_describe": LgAlikedDescribeIO}


# lg_preprocess_plan / lg_preprocess_resize (include/lightglue_amd.h)
LG_PREPROCESS_MAX_TAPS, LG_PREPROCESS_MAX_SIDE, LG_RESIZE_EDGE = 33, 2 ** 23, -1
LG_SIDE = {"long": 0, "short": 1, "vert": 2, "horz": 3}
LG_DTYPE_F32, LG_DTYPE_U8 = 0, 1
LG_PREPROCESS_RAGGED_MAX_BATCH = 256


class LgResizePlan(C.Structure):
    """lg_resize_plan (include/lightglue_amd.h)"""
    _fields_ = [
        ("h_in", C.c_int32), ("w_in", C.c_int32), ("h_out", C.c_int32), ("w_out", C.c_int32),
        ("ks_y", C.c_int32), ("ks_x", C.c_int32), ("align_corners", C.c_int32), ("identity", C.c_int32),
        ("sigma_y", C.c_double), ("sigma_x", C.c_double), ("scale_x", C.c_double), ("scale_y", C.c_double),
    ]


class LgImageSource(C.Structure):
    """lg_image_source (include/lightglue_amd.h): one image of a ragged preprocess call"""
    _fields_ = [
        ("data", C.c_void_p), ("dtype", C.c_int32), ("channels", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("stride_b", C.c_int64), ("stride_c", C.c_int64), ("stride_y", C.c_int64), ("stride_x", C.c_int64),
    ]


def wire_width(n0: int, n1: int) -> int:
    """LG_WIRE_WIDTH: int32 elements of one lg_forward_io.wire row"""
    return 3 * n0 + 3 * n1 + 2


class LightGlueAmdError(RuntimeError):
    pass


_lib = None


def library_path() -> Path:
    return _LIB_PATH


def load() -> C.CDLL:
    """Load the HIP library (once).  Raises if it has not been built — never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise LightGlueAmdError(
            f"{_LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            f"or `make -C {_LIB_PATH.parent / 'csrc'}`; lightglue_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(os.fspath(_LIB_PATH))
    lib.lg_last_error.restype = C.c_char_p
    lib.lg_version.restype = C.c_char_p
    lib.lg_engine_create.argtypes = [C.POINTER(LgConfig), C.POINTER(C.c_void_p)]
    lib.lg_engine_destroy.argtypes = [C.c_void_p]
    lib.lg_engine_destroy.restype = None
    lib.lg_engine_set_weight.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.POINTER(C.c_int64), C.c_int32]
    lib.lg_engine_finalize_weights.argtypes = [C.c_void_p]
    lib.lg_engine_reserve.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lib.lg_engine_forward.argtypes = [C.c_void_p, C.POINTER(LgForwardIO), C.c_void_p]
    lib.lg_unpack_wire.argtypes = [C.POINTER(LgUnpackIO), C.c_void_p]
    lib.lg_engine_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    lib.lg_engine_debug_stop_after.argtypes = [C.c_void_p, C.c_int32]
    lib.lg_engine_debug_read.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.lg_engine_debug_caps.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.lg_profile_num_classes.restype = C.c_int32
    lib.lg_profile_class_name.restype = C.c_char_p
    lib.lg_profile_class_name.argtypes = [C.c_int32]
    lib.lg_engine_profile_enable.argtypes = [C.c_void_p, C.c_int32]
    lib.lg_engine_profile_read.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int32]
    lib.lg_sp_detect_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lg_sp_detect_workspace_bytes.restype = C.c_int64
    lib.lg_sp_pack_conv_weight.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.lg_sp_encode_workspace_bytes.argtypes = [C.c_int32] * 3
    lib.lg_sp_encode_workspace_bytes.restype = C.c_int64
    lib.lg_sp_pack_conv_weight_split.argtypes = lib.lg_sp_pack_conv_weight.argtypes
    lib.lg_aliked_packed_bytes.argtypes = [C.c_int32]
    lib.lg_aliked_packed_bytes.restype = C.c_int64
    lib.lg_aliked_pack_weights.argtypes = [C.c_int32, C.POINTER(C.c_void_p), C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    lib.lg_aliked_levels_bytes.argtypes = [C.c_int32] * 3
    lib.lg_aliked_levels_bytes.restype = C.c_int64
    lib.lg_aliked_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lg_aliked_workspace_bytes.restype = C.c_int64
    lib.lg_aliked_detect_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lg_aliked_detect_workspace_bytes.restype = C.c_int64
    lib.lg_aliked_describe_workspace_bytes.argtypes = [C.c_int32] * 2
    lib.lg_aliked_describe_workspace_bytes.restype = C.c_int64
    lib.lg_preprocess_plan.argtypes = [C.c_int32] * 7 + [C.POINTER(LgResizePlan)]
    lib.lg_preprocess_resize.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.c_int64] * 4 + [C.POINTER(LgResizePlan), C.c_void_p, C.c_void_p]
    lib.lg_preprocess_ragged_table_bytes.argtypes = [C.c_int32]
    lib.lg_preprocess_ragged_table_bytes.restype = C.c_int64
    lib.lg_preprocess_ragged_plan.argtypes = ([C.POINTER(LgImageSource), C.POINTER(LgResizePlan)] + [C.c_int32] * 4 + [C.c_void_p, C.c_int64]
                                              + [C.POINTER(C.c_int64)] * 2 + [C.POINTER(C.c_int32)] * 2)
    lib.lg_preprocess_resize_ragged.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.lg_rootsift.argtypes = [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.lg_sift_filter_workspace_bytes.argtypes = [C.c_int32] * 4
    lib.lg_sift_filter_workspace_bytes.restype = C.c_int64
    lib.lg_sift_filter.argtypes = [C.c_void_p] * 6 + [C.c_int32] * 5 + [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.lg_nn_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    lib.lg_nn_workspace_bytes.restype = C.c_int64
    lib.lg_nn_match.argtypes = [C.POINTER(LgNnIO), C.c_void_p]
    lib.lg_twoview_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_uint32]
    lib.lg_twoview_workspace_bytes.restype = C.c_int64
    lib.lg_twoview_verify.argtypes = [C.POINTER(LgTwoViewIO), C.c_void_p]
    lib.lg_relpose_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_uint32]
    lib.lg_relpose_workspace_bytes.restype = C.c_int64
    lib.lg_relpose_estimate.argtypes = [C.POINTER(LgRelPoseIO), C.c_void_p]
    lib.lg_abspose_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32, C.c_uint32]
    lib.lg_abspose_workspace_bytes.restype = C.c_int64
    lib.lg_abspose_estimate.argtypes = [C.POINTER(LgAbsposeIO), C.c_void_p]
    lib.lg_triangulate_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_uint32]
    lib.lg_triangulate_workspace_bytes.restype = C.c_int64
    lib.lg_triangulate.argtypes = [C.POINTER(LgTriangulateIO), C.c_void_p]
    lib.lg_triangulate_robust_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int32]
    lib.lg_triangulate_robust_workspace_bytes.restype = C.c_int64
    lib.lg_triangulate_robust.argtypes = [C.POINTER(LgTriangulateRobustIO), C.c_void_p]
    lib.lg_bundle_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_uint32]
    lib.lg_bundle_workspace_bytes.restype = C.c_int64
    lib.lg_bundle_adjust.argtypes = [C.POINTER(LgBundleIO), C.c_void_p]
    lib.lg_bundle_robust_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_uint32]
    lib.lg_bundle_robust_workspace_bytes.restype = C.c_int64
    lib.lg_bundle_adjust_robust.argtypes = [C.POINTER(LgBundleRobustIO), C.c_void_p]
    lib.lg_bundle_focal_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_uint32]
    lib.lg_bundle_focal_workspace_bytes.restype = C.c_int64
    lib.lg_bundle_adjust_focal.argtypes = [C.POINTER(LgBundleFocalIO), C.c_void_p]
    lib.lg_bundle_pcg_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_uint32]
    lib.lg_bundle_pcg_workspace_bytes.restype = C.c_int64
    lib.lg_bundle_adjust_pcg.argtypes = [C.POINTER(LgBundlePcgIO), C.c_void_p]
    lib.lg_posegraph_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_uint32]
    lib.lg_posegraph_workspace_bytes.restype = C.c_int64
    lib.lg_posegraph_solve.argtypes = [C.POINTER(LgPosegraphIO), C.c_void_p]
    lib.lg_posegraph_pcg_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_uint32]
    lib.lg_posegraph_pcg_workspace_bytes.restype = C.c_int64
    lib.lg_posegraph_solve_pcg.argtypes = [C.POINTER(LgPosegraphPcgIO), C.c_void_p]
    lib.lg_positioning_workspace_bytes.argtypes = [C.c_int64, C.c_int32, C.c_int64, C.c_uint32]
    lib.lg_positioning_workspace_bytes.restype = C.c_int64
    lib.lg_positioning_solve.argtypes = [C.POINTER(LgPositioningIO), C.c_void_p]
    for fn, io in EXTRACT_STAGES.items():      # the six extractor stages: lg_<stage>(const lg_<stage>_io*, hipStream_t)
        getattr(lib, fn).argtypes = [C.POINTER(io), C.c_void_p]
    lib.lg_debug_mfma_sustained.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p]
    _lib = lib
    return lib


def check(rc: int) -> None:
    """Map C error codes to the exception types the reference raises."""
    if rc == LG_OK:
        return
    msg = load().lg_last_error().decode()
    if rc == LG_ERR_INVALID:
        raise AssertionError(msg)
    raise LightGlueAmdError(f"lightglue_amd error {rc}: {msg}")
