"""ctypes binding of libfisher_rast.so (C ABI declared in include/fisher_rast.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc --offload-arch=gfx950).  There is no
CPU fallback: if the shared object is missing, loading raises and every op of the package fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# FISHER_RAST_SO lets an A/B benchmark load another build of the same ABI; the default is the in-tree library
SO_PATH = os.environ.get("FISHER_RAST_SO", os.path.join(_HERE, "libfisher_rast.so"))

FR_OK, FR_EINVAL, FR_ELAUNCH, FR_ENOSPACE = 0, 1, 2, 3
FR_POPGS_TOPT, FR_POPGS_DOPT = 0, 1

_f32p = ctypes.c_void_p  # device pointers travel as raw addresses


class RasterCfg(ctypes.Structure):
    _fields_ = [
        ("P", ctypes.c_int32),
        ("image_height", ctypes.c_int32),
        ("image_width", ctypes.c_int32),
        ("tanfovx", ctypes.c_float),
        ("tanfovy", ctypes.c_float),
        ("scale_modifier", ctypes.c_float),
        ("sh_degree", ctypes.c_int32),
        ("sh_coeffs", ctypes.c_int32),
        ("prefiltered", ctypes.c_int32),
        ("bg", _f32p),
        ("viewmatrix", _f32p),
        ("projmatrix", _f32p),
        ("campos", _f32p),
    ]


class Gaussians(ctypes.Structure):
    _fields_ = [
        ("means3D", _f32p),
        ("colors_precomp", _f32p),
        ("shs", _f32p),
        ("opacities", _f32p),
        ("scales", _f32p),
        ("rotations", _f32p),
        ("cov3D_precomp", _f32p),
    ]


class FisherCfg(ctypes.Structure):
    _fields_ = [
        ("n_views", ctypes.c_int32),
        ("columns", ctypes.c_int32),
        ("dL_dpix", ctypes.c_float),
        ("w2c", _f32p),
        ("H_inv", _f32p),
        ("H_inv_view_stride", ctypes.c_int64),
        ("out_scores", _f32p),
        ("out_H", _f32p),
        ("out_H_view_stride", ctypes.c_int64),
        ("out_vis_count", ctypes.c_void_p),
        ("out_num_rendered", ctypes.c_void_p),
        ("dL_dpix_image", _f32p),
        ("dL_image_view_stride", ctypes.c_int64),
        ("tile_capacity", ctypes.c_int32),
        ("poses_are_c2w", ctypes.c_int32),
        ("reuse_static", ctypes.c_int32),
        ("order", ctypes.c_void_p),
        ("view_is_identity", ctypes.c_int32),
    ]


class OccCfg(ctypes.Structure):
    """fr_occ_cfg (include/fisher_occ.h)"""
    _fields_ = [
        ("grid_w", ctypes.c_int32),
        ("grid_h", ctypes.c_int32),
        ("cell_size", ctypes.c_float),
        ("center_x", ctypes.c_float),
        ("center_z", ctypes.c_float),
        ("height_lower", ctypes.c_float),
        ("height_upper", ctypes.c_float),
        ("far_distance", ctypes.c_float),
    ]


FR_LOSS_L1_SUM, FR_LOSS_L1_MEAN, FR_LOSS_L1_MASKED_MEAN = 0, 1, 2


class ImageLossCfg(ctypes.Structure):
    """fr_image_loss_cfg (include/fisher_rast.h)"""
    _fields_ = [
        ("C", ctypes.c_int32),
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("w_l1", ctypes.c_float),
        ("w_ssim", ctypes.c_float),
        ("l1_denom", ctypes.c_int32),
        ("mask_channels", ctypes.c_int32),
        ("mask_weights_ssim_map", ctypes.c_int32),
    ]


FR_INGEST_NONPRESENCE, FR_INGEST_MASK = 0, 1
FR_INGEST_STATUS_WORDS = 5
FR_INGEST_WS_INDEX_OFFSET = 8192


class FrameIngestCfg(ctypes.Structure):
    """fr_frame_ingest_cfg (include/fisher_rast.h)"""
    _fields_ = [
        ("H", ctypes.c_int32),
        ("W", ctypes.c_int32),
        ("downsample", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("sil_thres", ctypes.c_float),
        ("depth_error_ratio", ctypes.c_float),
        ("transform_pts", ctypes.c_int32),
        ("scale_cols", ctypes.c_int32),
        ("means_stride", ctypes.c_int32),
        ("colors_stride", ctypes.c_int32),
        ("intrinsics", _f32p),
    ]


FR_EDIT_COPY, FR_EDIT_ZERO = 0, 1
FR_EDIT_STATUS_WORDS = 4
FR_EDIT_MAX_ARRAYS = 32
FR_EDIT_MAX_COLS = 16


def edit_ws_list_stride(P):
    """FR_EDIT_WS_LIST_STRIDE (include/fisher_rast.h): list k of the map-edit workspace begins at byte k * this"""
    return (int(P) * 4 + 15) & ~15


class MapEditArray(ctypes.Structure):
    """fr_map_edit_array (include/fisher_rast.h)"""
    _fields_ = [
        ("src", ctypes.c_void_p),
        ("dst", ctypes.c_void_p),
        ("cols", ctypes.c_int32),
        ("appended", ctypes.c_int32),
    ]


FR_ADAM_MAX_ARRAYS = 16


class AdamArray(ctypes.Structure):
    """fr_adam_array (include/fisher_rast.h)"""
    _fields_ = [
        ("param", ctypes.c_void_p),
        ("grad", ctypes.c_void_p),
        ("exp_avg", ctypes.c_void_p),
        ("exp_avg_sq", ctypes.c_void_p),
        ("n", ctypes.c_int64),
        ("w1", ctypes.c_float),
        ("beta2", ctypes.c_float),
        ("c2", ctypes.c_float),
        ("bc2_sqrt", ctypes.c_float),
        ("eps", ctypes.c_float),
        ("neg_step_size", ctypes.c_float),
        ("fresh", ctypes.c_int32),
    ]


class RenderVarCfg(ctypes.Structure):
    """fr_rendervar_cfg (include/fisher_rast.h)"""
    _fields_ = [("P", ctypes.c_int32), ("scale_cols", ctypes.c_int32), ("time_idx", ctypes.c_int32), ("n_frames", ctypes.c_int32)] + \
               [(n, ctypes.c_void_p) for n in (
                   "cam_unnorm_rots", "cam_trans", "first_frame_w2c", "means3D", "unnorm_rotations", "logit_opacities", "log_scales",
                   "pts", "feats", "rotations", "opacities", "scales", "rel_w2c",
                   "g_pts", "g_feats", "g_rotations", "g_opacities", "g_scales",
                   "g_means3D", "g_unnorm_rotations", "g_logit_opacities", "g_log_scales", "g_cam_unnorm_rots", "g_cam_trans")]


FR_KEYFRAME_STATUS_WORDS = 4
FR_KEYFRAME_MAX_POINTS = 4096


class KeyframeCfg(ctypes.Structure):
    """fr_keyframe_cfg (include/fisher_rast.h)"""
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("edge", ctypes.c_int32),
                ("n_valid_idx", ctypes.c_int32), ("intrinsics", _f32p), ("w2c", _f32p)]


FR_CLOUD_MAX_POINTS = 1 << 27
FR_CLOUD_STATS_WORDS = 4
FR_CLOUD_SOURCE_POINTS, FR_CLOUD_SOURCE_DEPTH = 0, 1


class CloudQueryCfg(ctypes.Structure):
    """fr_cloud_query_cfg (include/fisher_rast.h)"""
    _fields_ = [("source", ctypes.c_int32), ("M", ctypes.c_int32), ("H", ctypes.c_int32), ("W", ctypes.c_int32), ("stride", ctypes.c_int32),
                ("flip_z", ctypes.c_int32), ("dist_th", ctypes.c_float)] + \
               [(n, ctypes.c_void_p) for n in ("queries", "depth", "kinv", "c2w", "out_dist", "out_idx", "out_flag", "out_stats")]


FR_CLUSTER_MAX_POINTS = 1 << 26
FR_DBSCAN_STATUS_WORDS = 8
FR_TARGET_STATUS_WORDS = 16

FR_EVAL_ROW = 8
FR_EVAL_GT_F32_CHW, FR_EVAL_GT_U8_HWC = 0, 1


class ViewMetricsCfg(ctypes.Structure):
    """fr_view_metrics_cfg (include/fisher_rast.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("V", "H", "W", "gt_layout", "gt_channels", "clamp_render", "depth_valid_only")] + \
               [(n, ctypes.c_int64) for n in ("render_view_stride", "depth_view_stride", "gt_depth_view_stride")]


FR_LOSS_MASK_STATUS_WORDS = 5
FR_OUTSIDE_STATUS_WORDS = 6


class LossMaskCfg(ctypes.Structure):
    """fr_loss_mask_cfg (include/fisher_rast.h)"""
    _fields_ = [("H", ctypes.c_int32), ("W", ctypes.c_int32), ("sil_thres", ctypes.c_float), ("reject_outliers", ctypes.c_int32),
                ("outlier_ratio", ctypes.c_float), ("need_presence", ctypes.c_int32)]


FR_PLAN_STATUS_WORDS = 4
FR_PLAN_TILE = 64
FR_PLAN_UNREACHED = 0xFFFFFFFFFFFFFFFF
FR_ACTION_MAX_QUEUE = 128
FR_ACTION_OBJECT_MAX = 200


# every symbol include/fisher_rast.h and include/fisher_occ.h declare
EXPORTS = (
    "fr_version", "fr_last_error", "fr_build_id", "fr_init", "fr_fisher_workspace_layout", "fr_fisher_part_list_offset", "fr_workspace_bytes", "fr_workspace_layout", "fr_mark_visible",
    "fr_forward", "fr_backward", "fr_backward_scratch_bytes", "fr_backward_ws", "fr_forward_pair", "fr_forward_features", "fr_backward_pair", "fr_backward_pair_scratch_bytes", "fr_backward_pair_ws", "fr_fisher_workspace_bytes", "fr_fisher_views",
    "fr_fisher_pose_workspace_bytes", "fr_fisher_pose_workspace_layout", "fr_fisher_pose_views",
    "fr_render_views_workspace_bytes", "fr_render_views_workspace_layout", "fr_render_views",
    "fr_fisher_point_workspace_bytes", "fr_fisher_point_workspace_layout", "fr_fisher_point_views",
    "fr_popgs_diag_criterion_workspace_bytes", "fr_popgs_diag_criterion",
    "fr_image_loss_workspace_bytes", "fr_image_loss_forward", "fr_image_loss_backward",
    "fr_frame_ingest_workspace_bytes", "fr_frame_ingest_select", "fr_frame_ingest_emit",
    "fr_map_edit_workspace_bytes", "fr_map_edit_plan", "fr_map_edit_apply", "fr_map_edit_split_children", "fr_adam_step",
    "fr_rendervar_workspace_bytes", "fr_rendervar_forward", "fr_rendervar_backward",
    "fr_keyframe_valid_pixels_workspace_bytes", "fr_keyframe_overlap_workspace_bytes", "fr_keyframe_valid_pixels", "fr_keyframe_overlap",
    "fr_densify_stats", "fr_densify_masks", "fr_prune_mask", "fr_knn_workspace_bytes", "fr_knn_dist2", "fr_spatial_order_workspace_bytes", "fr_spatial_order", "fr_profile_enable", "fr_profile_fetch",
    "fr_occ_workspace_bytes", "fr_occ_update", "fr_occ_freespace", "fr_occ_frontiers", "fr_occ_erode", "fr_occ_cells_of",
    "fr_occ_ring_candidates", "fr_occ_free_candidates",
    "fr_plan_workspace_bytes", "fr_plan_round_cap", "fr_plan_grid", "fr_plan_tiers", "fr_plan_field", "fr_plan_paths",
    "fr_plan_actions", "fr_rollout_actions", "fr_plan_actions_object",
    "fr_occ_object_cells", "fr_occ_grid_candidates",
    "fr_cloud_index_bytes", "fr_cloud_index_workspace_bytes", "fr_cloud_query_workspace_bytes", "fr_cloud_index_build", "fr_cloud_query",
    "fr_dbscan_workspace_bytes", "fr_target_select_workspace_bytes", "fr_dbscan", "fr_target_select",
    "fr_view_metrics_workspace_bytes", "fr_view_metrics", "fr_view_metrics_summary",
    "fr_loss_mask_workspace_bytes", "fr_loss_mask", "fr_bg_penalty_workspace_bytes", "fr_bg_penalty_forward", "fr_bg_penalty_backward",
    "fr_outside_mask_workspace_bytes", "fr_outside_mask",
)

_lib = None

_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")
SOURCES = [os.path.join(_CSRC, n) for n in ("fisher_rast.hip", "fisher_occ.hip", "fr_popgs.hip", "fr_loss.hip", "fr_ingest.hip", "fr_mapedit.hip", "fr_adam.hip", "fr_rendervar.hip", "fr_keyframe.hip", "fr_plan.hip", "fr_action.hip", "fr_action_object.hip", "fr_goal.hip", "fr_cloud.hip", "fr_cluster.hip", "fr_eval.hip", "fr_objloss.hip", "fr_math.h", "fr_rig.inc",
                                                  "fr_loss_math.h", "fr_ingest_math.h", "fr_mapedit_math.h", "fr_adam_math.h", "fr_rendervar_math.h", "fr_keyframe_math.h", "fr_plan_math.h", "fr_action_math.h", "fr_action_object_math.h", "fr_goal_math.h", "fr_cloud_math.h", "fr_cluster_math.h", "fr_eval_math.h", "fr_objloss_math.h", "fr_internal.h", "fr_block.h", "fr_ssim_tile.h")] + \
          [os.path.join(_INCLUDE, n) for n in ("fisher_rast.h", "fisher_occ.h")]


def source_hash():
    """sha256 (first 16 hex digits) over the kernel and header sources, or None when they are not beside the package."""
    import hashlib
    h = hashlib.sha256()
    for f in SOURCES:
        if not os.path.exists(f):
            return None
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


class FisherRastError(RuntimeError):
    pass


def load():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise FisherRastError(
            f"{SO_PATH} is missing: the HIP extension has not been built "
            "(run `python -c \"import __graft_entry__ as g; g.build()\"` at the repo root). "
            "There is no CPU fallback for this path.")
    # PyTorch-ROCm ships its own HIP runtime; it has to be the one already in the process when this library's
    # libamdhip64 dependency is resolved, or the two would each hold their own (device-less) state.
    import torch  # noqa: F401
    lib = ctypes.CDLL(SO_PATH)
    ab_build = "FISHER_RAST_SO" in os.environ          # an A/B partner may be an older build, without the newest entry points
    for name in EXPORTS:
        if not hasattr(lib, name) and not ab_build:
            raise FisherRastError(f"{SO_PATH} does not export {name}")
    lib.fr_version.restype = ctypes.c_int
    lib.fr_last_error.restype = ctypes.c_char_p
    lib.fr_build_id.restype = ctypes.c_char_p
    lib.fr_init.restype = ctypes.c_int
    lib.fr_fisher_workspace_layout.restype = ctypes.c_int
    lib.fr_fisher_workspace_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                               ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
    if hasattr(lib, "fr_fisher_part_list_offset"):
        lib.fr_fisher_part_list_offset.restype = ctypes.c_int
        lib.fr_fisher_part_list_offset.argtypes = lib.fr_fisher_workspace_layout.argtypes
    # a stale or foreign binary must not pass for the sources beside it (FISHER_RAST_SO builds for A/B runs are exempt)
    want = source_hash()
    got = lib.fr_build_id().decode().split(":")[-1]
    if "FISHER_RAST_SO" not in os.environ and want is not None and got != want:
        raise FisherRastError(f"{SO_PATH} was built from other sources (build id {got}, sources {want}): "
                              "run `python -c \"import __graft_entry__ as g; g.build()\"`")
    lib.fr_workspace_bytes.restype = ctypes.c_int
    lib.fr_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_size_t)]
    lib.fr_workspace_layout.restype = ctypes.c_int
    lib.fr_workspace_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                        ctypes.POINTER(ctypes.c_size_t)]
    lib.fr_mark_visible.restype = ctypes.c_int
    lib.fr_mark_visible.argtypes = [ctypes.c_int32, _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_forward.restype = ctypes.c_int
    lib.fr_forward.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians),
                               ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                               _f32p, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_backward.restype = ctypes.c_int
    lib.fr_backward.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.c_void_p,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                _f32p, ctypes.c_int32] + [_f32p] * 9 + [ctypes.c_void_p]
    lib.fr_backward_scratch_bytes.restype = ctypes.c_size_t
    lib.fr_backward_scratch_bytes.argtypes = [ctypes.c_int32] * 4 + [ctypes.c_int64]
    lib.fr_backward_ws.restype = ctypes.c_int
    lib.fr_backward_ws.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                   _f32p, ctypes.c_int32] + [_f32p] * 9 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_forward_pair.restype = ctypes.c_int
    lib.fr_forward_pair.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), _f32p,
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                    _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_forward_features.restype = ctypes.c_int
    lib.fr_forward_features.argtypes = [ctypes.POINTER(RasterCfg), _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        _f32p, ctypes.c_void_p]
    lib.fr_backward_pair.restype = ctypes.c_int
    lib.fr_backward_pair.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     _f32p, _f32p, _f32p] + [_f32p] * 10 + [ctypes.c_void_p]
    lib.fr_backward_pair_scratch_bytes.restype = ctypes.c_size_t
    lib.fr_backward_pair_scratch_bytes.argtypes = [ctypes.c_int32] * 3 + [ctypes.c_int64]
    lib.fr_backward_pair_ws.restype = ctypes.c_int
    lib.fr_backward_pair_ws.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        _f32p, _f32p, _f32p] + [_f32p] * 10 + [ctypes.c_int64, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_fisher_workspace_bytes.restype = ctypes.c_size_t
    lib.fr_fisher_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_int64, ctypes.c_int32]
    lib.fr_fisher_views.restype = ctypes.c_int
    lib.fr_fisher_views.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians),
                                    ctypes.POINTER(FisherCfg), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64,
                                    ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_fisher_pose_workspace_bytes.restype = ctypes.c_size_t
    lib.fr_fisher_pose_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
    lib.fr_fisher_pose_workspace_layout.restype = ctypes.c_int
    lib.fr_fisher_pose_workspace_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                    ctypes.POINTER(ctypes.c_size_t)]
    lib.fr_fisher_pose_views.restype = ctypes.c_int
    lib.fr_fisher_pose_views.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.POINTER(FisherCfg), _f32p,
                                         ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_render_views"):
        lib.fr_render_views_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_render_views_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64]
        lib.fr_render_views_workspace_layout.restype = ctypes.c_int
        lib.fr_render_views_workspace_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                         ctypes.POINTER(ctypes.c_size_t)]
        lib.fr_render_views.restype = ctypes.c_int
        lib.fr_render_views.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.POINTER(FisherCfg),
                                        _f32p, _f32p, _f32p, _f32p,
                                        ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_fisher_point_views"):
        lib.fr_fisher_point_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_fisher_point_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                        ctypes.c_int32]
        lib.fr_fisher_point_workspace_layout.restype = ctypes.c_int
        lib.fr_fisher_point_workspace_layout.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                                         ctypes.c_int32, ctypes.POINTER(ctypes.c_size_t)]
        lib.fr_fisher_point_views.restype = ctypes.c_int
        lib.fr_fisher_point_views.argtypes = [ctypes.POINTER(RasterCfg), ctypes.POINTER(Gaussians), ctypes.POINTER(FisherCfg), _f32p, _f32p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_popgs_diag_criterion"):
        lib.fr_popgs_diag_criterion_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_popgs_diag_criterion_workspace_bytes.argtypes = [ctypes.c_int32, ctypes.c_int64]
        lib.fr_popgs_diag_criterion.restype = ctypes.c_int
        lib.fr_popgs_diag_criterion.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64, _f32p, _f32p, ctypes.c_int64, _f32p,
                                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p,
                                                ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    if hasattr(lib, "fr_image_loss_forward"):
        lib.fr_image_loss_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_image_loss_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        lib.fr_image_loss_forward.restype = ctypes.c_int
        lib.fr_image_loss_forward.argtypes = [ctypes.POINTER(ImageLossCfg), _f32p, _f32p, ctypes.c_void_p, _f32p, _f32p, _f32p, _f32p,
                                              ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_image_loss_backward.restype = ctypes.c_int
        lib.fr_image_loss_backward.argtypes = [ctypes.POINTER(ImageLossCfg), _f32p, _f32p, ctypes.c_void_p, _f32p, _f32p, _f32p, ctypes.c_void_p]
    if hasattr(lib, "fr_frame_ingest_select"):
        lib.fr_frame_ingest_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_frame_ingest_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        lib.fr_frame_ingest_select.restype = ctypes.c_int
        lib.fr_frame_ingest_select.argtypes = [ctypes.POINTER(FrameIngestCfg), _f32p, _f32p, ctypes.c_void_p, ctypes.c_void_p,
                                               ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_frame_ingest_emit.restype = ctypes.c_int
        lib.fr_frame_ingest_emit.argtypes = [ctypes.POINTER(FrameIngestCfg), _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_int32,
                                             ctypes.c_int64] + [_f32p] * 6 + [ctypes.c_void_p]
    if hasattr(lib, "fr_map_edit_plan"):
        lib.fr_map_edit_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_map_edit_workspace_bytes.argtypes = [ctypes.c_int32]
        lib.fr_map_edit_plan.restype = ctypes.c_int
        lib.fr_map_edit_plan.argtypes = [ctypes.c_int32] + [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_map_edit_apply.restype = ctypes.c_int
        lib.fr_map_edit_apply.argtypes = [ctypes.POINTER(MapEditArray)] + [ctypes.c_int32] * 6 + [ctypes.c_void_p, ctypes.c_void_p]
        lib.fr_map_edit_split_children.restype = ctypes.c_int
        lib.fr_map_edit_split_children.argtypes = [ctypes.c_int32] * 3 + [_f32p] * 4 + [ctypes.c_void_p]
    if hasattr(lib, "fr_adam_step"):
        lib.fr_adam_step.restype = ctypes.c_int
        lib.fr_adam_step.argtypes = [ctypes.POINTER(AdamArray), ctypes.c_int32, ctypes.c_void_p]
    if hasattr(lib, "fr_rendervar_forward"):
        lib.fr_rendervar_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_rendervar_workspace_bytes.argtypes = [ctypes.c_int32]
        lib.fr_rendervar_forward.restype = ctypes.c_int
        lib.fr_rendervar_forward.argtypes = [ctypes.POINTER(RenderVarCfg), ctypes.c_void_p]
        lib.fr_rendervar_backward.restype = ctypes.c_int
        lib.fr_rendervar_backward.argtypes = [ctypes.POINTER(RenderVarCfg), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    if hasattr(lib, "fr_keyframe_overlap"):
        lib.fr_keyframe_valid_pixels_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_keyframe_valid_pixels_workspace_bytes.argtypes = [ctypes.c_int32] * 2
        lib.fr_keyframe_overlap_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_keyframe_overlap_workspace_bytes.argtypes = [ctypes.c_int32]
        lib.fr_keyframe_valid_pixels.restype = ctypes.c_int
        lib.fr_keyframe_valid_pixels.argtypes = [ctypes.c_int32, ctypes.c_int32, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                                 ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_keyframe_overlap.restype = ctypes.c_int
        lib.fr_keyframe_overlap.argtypes = [ctypes.POINTER(KeyframeCfg), _f32p, ctypes.c_void_p, ctypes.c_void_p, _f32p, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_void_p, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                            ctypes.c_void_p]
    lib.fr_densify_stats.restype = ctypes.c_int
    lib.fr_densify_stats.argtypes = [ctypes.c_int32, ctypes.c_void_p, _f32p, _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_densify_masks.restype = ctypes.c_int
    lib.fr_densify_masks.argtypes = [ctypes.c_int32, _f32p, _f32p, _f32p, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_prune_mask.restype = ctypes.c_int
    lib.fr_prune_mask.argtypes = [ctypes.c_int32, _f32p, _f32p, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_knn_workspace_bytes.restype = ctypes.c_size_t
    lib.fr_knn_workspace_bytes.argtypes = [ctypes.c_int32]
    lib.fr_knn_dist2.restype = ctypes.c_int
    lib.fr_knn_dist2.argtypes = [ctypes.c_int32, _f32p, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_spatial_order_workspace_bytes.restype = ctypes.c_size_t
    lib.fr_spatial_order_workspace_bytes.argtypes = [ctypes.c_int32]
    lib.fr_spatial_order.restype = ctypes.c_int
    lib.fr_spatial_order.argtypes = [ctypes.c_int32, _f32p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_profile_enable.restype = ctypes.c_int
    lib.fr_profile_enable.argtypes = [ctypes.c_int]
    lib.fr_profile_fetch.restype = ctypes.c_int
    lib.fr_profile_fetch.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.c_int]
    occp = ctypes.POINTER(OccCfg)
    f4, f16 = ctypes.c_float * 4, ctypes.c_float * 16
    lib.fr_occ_workspace_bytes.restype = ctypes.c_size_t
    lib.fr_occ_workspace_bytes.argtypes = [occp]
    lib.fr_occ_update.restype = ctypes.c_int
    lib.fr_occ_update.argtypes = [occp, _f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(f4), ctypes.POINTER(f16),
                                  ctypes.POINTER(ctypes.c_float), ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _f32p,
                                  ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_occ_freespace.restype = ctypes.c_int
    lib.fr_occ_freespace.argtypes = [occp, _f32p, _f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_occ_frontiers.restype = ctypes.c_int
    lib.fr_occ_frontiers.argtypes = [occp, _f32p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_occ_erode.restype = ctypes.c_int
    lib.fr_occ_erode.argtypes = [occp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    lib.fr_occ_ring_candidates.restype = ctypes.c_int
    lib.fr_occ_ring_candidates.argtypes = [occp, _f32p, ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                           ctypes.c_uint32, ctypes.c_void_p, ctypes.c_int32, _f32p, ctypes.c_void_p, ctypes.c_void_p]
    lib.fr_occ_free_candidates.restype = ctypes.c_int
    lib.fr_occ_free_candidates.argtypes = [occp, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint32, _f32p, ctypes.c_int32,
                                           ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    lib.fr_occ_cells_of.restype = ctypes.c_int
    lib.fr_occ_cells_of.argtypes = [occp, _f32p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_plan_field"):
        lib.fr_plan_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_plan_workspace_bytes.argtypes = [occp]
        lib.fr_plan_round_cap.restype = ctypes.c_int32
        lib.fr_plan_round_cap.argtypes = [occp]
        lib.fr_plan_grid.restype = ctypes.c_int
        lib.fr_plan_grid.argtypes = [occp, _f32p, _f32p, ctypes.c_int32, ctypes.c_float, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_plan_tiers.restype = ctypes.c_int
        lib.fr_plan_tiers.argtypes = [occp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        lib.fr_plan_field.restype = ctypes.c_int
        lib.fr_plan_field.argtypes = [occp, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.POINTER(ctypes.c_int32 * 2), ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_plan_paths.restype = ctypes.c_int
        lib.fr_plan_paths.argtypes = [occp, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32,
                                      ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_plan_actions"):
        vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
        f64p = ctypes.POINTER(ctypes.c_double)
        lib.fr_plan_actions.restype = ctypes.c_int
        lib.fr_plan_actions.argtypes = [occp, vp, i32, vp, vp, vp, i32, f64p, f64, f64, f64, i32, f64, vp, vp, vp, vp, vp, vp, vp]
        lib.fr_rollout_actions.restype = ctypes.c_int
        lib.fr_rollout_actions.argtypes = [f64p, vp, vp, i32, i32, f64, f64, vp, vp, vp]
    if hasattr(lib, "fr_plan_actions_object"):
        vp, i32, f64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double, ctypes.c_float
        lib.fr_plan_actions_object.restype = ctypes.c_int
        lib.fr_plan_actions_object.argtypes = [occp, vp, i32, vp, vp, vp, i32, ctypes.POINTER(ctypes.c_double), f64, f64, f64, f64] + [vp] * 9
        lib.fr_occ_object_cells.restype = ctypes.c_int
        lib.fr_occ_object_cells.argtypes = [occp, vp, i32, i32, vp, i32, vp, vp, ctypes.c_size_t, vp]
        lib.fr_occ_grid_candidates.restype = ctypes.c_int
        lib.fr_occ_grid_candidates.argtypes = [occp, vp, i32, vp, vp, i32, f32, f32, i32, i32, i32, f32, ctypes.c_uint32, vp, i32, vp, vp, vp]
    if hasattr(lib, "fr_cloud_query"):
        for f in (lib.fr_cloud_index_bytes, lib.fr_cloud_index_workspace_bytes, lib.fr_cloud_query_workspace_bytes):
            f.restype = ctypes.c_size_t
            f.argtypes = [ctypes.c_int32]
        lib.fr_cloud_index_build.restype = ctypes.c_int
        lib.fr_cloud_index_build.argtypes = [ctypes.c_int32, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_cloud_query.restype = ctypes.c_int
        lib.fr_cloud_query.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int32, ctypes.POINTER(CloudQueryCfg), ctypes.c_void_p, ctypes.c_size_t,
                                       ctypes.c_void_p]
    if hasattr(lib, "fr_target_select"):
        for f in (lib.fr_dbscan_workspace_bytes, lib.fr_target_select_workspace_bytes):
            f.restype = ctypes.c_size_t
            f.argtypes = [ctypes.c_int32]
        lib.fr_dbscan.restype = ctypes.c_int
        lib.fr_dbscan.argtypes = [ctypes.c_int32, _f32p, ctypes.c_float, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_target_select.restype = ctypes.c_int
        lib.fr_target_select.argtypes = [ctypes.c_int32, _f32p, _f32p, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float,
                                         ctypes.c_int32] + [ctypes.c_void_p] * 7 + [ctypes.c_size_t, ctypes.c_void_p]
    if hasattr(lib, "fr_view_metrics"):
        lib.fr_view_metrics_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_view_metrics_workspace_bytes.argtypes = [ctypes.c_int32] * 3
        lib.fr_view_metrics.restype = ctypes.c_int
        lib.fr_view_metrics.argtypes = [ctypes.POINTER(ViewMetricsCfg)] + [ctypes.c_void_p] * 8 + [ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_view_metrics_summary.restype = ctypes.c_int
        lib.fr_view_metrics_summary.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    if hasattr(lib, "fr_loss_mask"):
        lib.fr_loss_mask_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_loss_mask_workspace_bytes.argtypes = [ctypes.c_int32] * 2
        lib.fr_loss_mask.restype = ctypes.c_int
        lib.fr_loss_mask.argtypes = [ctypes.POINTER(LossMaskCfg), _f32p, _f32p] + [ctypes.c_void_p] * 4 + [ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_bg_penalty_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_bg_penalty_workspace_bytes.argtypes = [ctypes.c_int32] * 2
        lib.fr_bg_penalty_forward.restype = ctypes.c_int
        lib.fr_bg_penalty_forward.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _f32p, _f32p, ctypes.c_void_p,
                                              _f32p, _f32p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        lib.fr_bg_penalty_backward.restype = ctypes.c_int
        lib.fr_bg_penalty_backward.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_float, ctypes.c_float, _f32p, _f32p, ctypes.c_void_p,
                                               _f32p, _f32p, _f32p, _f32p, ctypes.c_void_p]
        lib.fr_outside_mask_workspace_bytes.restype = ctypes.c_size_t
        lib.fr_outside_mask_workspace_bytes.argtypes = [ctypes.c_int32]
        lib.fr_outside_mask.restype = ctypes.c_int
        lib.fr_outside_mask.argtypes = [ctypes.c_int32, ctypes.c_int32, _f32p, _f32p, _f32p, _f32p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    _lib = lib
    return lib


def check(rc, what):
    if rc != FR_OK:
        msg = load().fr_last_error().decode("utf-8", "replace")
        raise FisherRastError(f"{what} failed (code {rc}): {msg}")
