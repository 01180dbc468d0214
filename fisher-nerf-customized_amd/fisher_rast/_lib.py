"""ctypes binding of libfisher_rast.so (C ABI declared in include/fisher_rast.h).

The library is built in-tree by `__graft_entry__.build()` (hipcc for gfx950, HIPCC_FLAGS there).  There is no
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


FR_EXT_POPGS_BLOCK = 1
FR_POPGS_BLOCK_VISIBLE, FR_POPGS_BLOCK_SCORE, FR_POPGS_BLOCK_PRIOR = 0, 1, 2
FR_POPGS_BLOCK_MAX_WG = 256


class RasterExt(ctypes.Structure):
    """fr_raster_ext (include/fisher_rast.h): with RasterCfg.ext set, fr_fisher_views is the POp-GS block stage"""
    _fields_ = [(n, ctypes.c_int32) for n in ("kind", "mode", "K", "use_opacity", "use_rot", "use_scale", "criterion", "n")] + \
               [("lam", ctypes.c_double)] + \
               [(n, ctypes.c_void_p) for n in ("vis_in", "out_vis", "out_vis_count", "prior_blocks", "prior_idx", "out_scores", "out_matched")]


def popgs_block_workspace_bytes(P, poses):
    """FR_POPGS_BLOCK_WS_BYTES (include/fisher_rast.h): the workspace of the block stage for `poses` poses of a map of P Gaussians"""
    P, poses = int(P), int(poses)
    a = lambda x: (x + 255) & ~255
    wgs = (P + 255) // 256
    return a(poses * P) + a(poses * P * 4) + 2 * a(poses * wgs * 4) + a(poses * 4) + a(poses * FR_POPGS_BLOCK_MAX_WG * 32)


def popgs_block_dim(use_opacity, use_rot, use_scale):
    """d of the d x d blocks: mean 3, opacity 1, rot 4, scale 3"""
    return 3 + (1 if use_opacity else 0) + (4 if use_rot else 0) + (3 if use_scale else 0)


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
        ("ext", ctypes.POINTER(RasterExt)),      # null (the default): every entry point as before the field existed
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
               [(n, ctypes.c_void_p) for n in ("queries", "depth", "kinv", "c2w", "out_dist", "out_idx", "out_flag", "out_stats")] + \
               [("seed_d2", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("flag_near", ctypes.c_int32), ("out_points", ctypes.c_void_p)]


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


def _prototypes():
    """{name: (restype, argtypes)} of every symbol include/fisher_rast.h and include/fisher_occ.h declare (tests/test_prototypes_cpu.py
    holds each row against its declaration); argtypes None = declared (void), left unset"""
    ci, cs, i32, i64, u32, sz = ctypes.c_int, ctypes.c_char_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_size_t
    f32, f64, vp, fp, P = ctypes.c_float, ctypes.c_double, ctypes.c_void_p, _f32p, ctypes.POINTER
    rc, gs, fc, occ = P(RasterCfg), P(Gaussians), P(FisherCfg), P(OccCfg)
    back = [rc, gs, vp, vp, vp, vp, fp, i32] + [fp] * 9                  # fr_backward and fr_backward_ws up to the gradients
    back_pair = [rc, gs, vp, vp, vp, vp, fp, fp, fp] + [fp] * 10         # the same of the pair forms
    own_ws = [i64, vp, sz, vp]                                           # the *_ws tail: capacity, workspace, bytes, stream
    return {
        "fr_version": (ci, None),
        "fr_last_error": (cs, None),
        "fr_build_id": (cs, None),
        "fr_init": (ci, None),
        "fr_fisher_workspace_layout": (ci, [i32, i32, i32, i32, i64, i32, P(sz)]),
        "fr_fisher_part_list_offset": (ci, [i32, i32, i32, i32, i64, i32, P(sz)]),
        "fr_workspace_bytes": (ci, [i32, i32, i32, i64, P(sz)]),
        "fr_workspace_layout": (ci, [i32, i32, i32, i64, P(sz)]),
        "fr_mark_visible": (ci, [i32, fp, fp, fp, vp, vp]),
        "fr_forward": (ci, [rc, gs, vp, vp, i64, vp, fp, fp, vp, vp, vp]),
        "fr_backward": (ci, back + [vp]),
        "fr_backward_scratch_bytes": (sz, [i32] * 4 + [i64]),
        "fr_backward_ws": (ci, back + own_ws),
        "fr_forward_pair": (ci, [rc, gs, fp, vp, vp, i64, vp, fp, fp, fp, vp, vp, vp]),
        "fr_forward_features": (ci, [rc, fp, vp, vp, vp, fp, vp]),
        "fr_backward_pair": (ci, back_pair + [vp]),
        "fr_backward_pair_scratch_bytes": (sz, [i32] * 3 + [i64]),
        "fr_backward_pair_ws": (ci, back_pair + own_ws),
        "fr_fisher_workspace_bytes": (sz, [i32, i32, i32, i32, i64, i32]),
        "fr_fisher_views": (ci, [rc, gs, fc, vp, sz, i64, vp, vp]),
        "fr_fisher_pose_workspace_bytes": (sz, [i32] * 4 + [i64]),
        "fr_fisher_pose_workspace_layout": (ci, [i32] * 4 + [i64, P(sz)]),
        "fr_fisher_pose_views": (ci, [rc, gs, fc, fp, vp, sz, i64, vp, vp]),
        "fr_render_views_workspace_bytes": (sz, [i32] * 4 + [i64]),
        "fr_render_views_workspace_layout": (ci, [i32] * 4 + [i64, P(sz)]),
        "fr_render_views": (ci, [rc, gs, fc, fp, fp, fp, fp, vp, sz, i64, vp, vp]),
        "fr_fisher_point_workspace_bytes": (sz, [i32] * 4 + [i64, i32]),
        "fr_fisher_point_workspace_layout": (ci, [i32] * 4 + [i64, i32, P(sz)]),
        "fr_fisher_point_views": (ci, [rc, gs, fc, fp, fp, vp, sz, i64, vp, vp]),
        "fr_popgs_diag_criterion_workspace_bytes": (sz, [i32, i64]),
        "fr_popgs_diag_criterion": (ci, [i32, i32, i64, fp, fp, i64, fp, vp, vp, f32, i32, vp, vp, sz, vp]),
        "fr_image_loss_workspace_bytes": (sz, [i32] * 3),
        "fr_image_loss_forward": (ci, [P(ImageLossCfg), fp, fp, vp, fp, fp, fp, fp, vp, sz, vp]),
        "fr_image_loss_backward": (ci, [P(ImageLossCfg), fp, fp, vp, fp, fp, fp, vp]),
        "fr_frame_ingest_workspace_bytes": (sz, [i32] * 3),
        "fr_frame_ingest_select": (ci, [P(FrameIngestCfg), fp, fp, vp, vp, vp, sz, vp]),
        "fr_frame_ingest_emit": (ci, [P(FrameIngestCfg), fp, fp, fp, vp, i32, i64] + [fp] * 6 + [vp]),
        "fr_map_edit_workspace_bytes": (sz, [i32]),
        "fr_map_edit_plan": (ci, [i32] + [vp] * 5 + [sz, vp]),
        "fr_map_edit_apply": (ci, [P(MapEditArray)] + [i32] * 6 + [vp, vp]),
        "fr_map_edit_split_children": (ci, [i32] * 3 + [fp] * 4 + [vp]),
        "fr_adam_step": (ci, [P(AdamArray), i32, vp]),
        "fr_rendervar_workspace_bytes": (sz, [i32]),
        "fr_rendervar_forward": (ci, [P(RenderVarCfg), vp]),
        "fr_rendervar_backward": (ci, [P(RenderVarCfg), vp, sz, vp]),
        "fr_keyframe_valid_pixels_workspace_bytes": (sz, [i32] * 2),
        "fr_keyframe_overlap_workspace_bytes": (sz, [i32]),
        "fr_keyframe_valid_pixels": (ci, [i32, i32, fp, vp, vp, vp, vp, sz, vp]),
        "fr_keyframe_overlap": (ci, [P(KeyframeCfg), fp, vp, vp, fp, vp, vp, vp, fp, vp, vp, sz, vp]),
        "fr_densify_stats": (ci, [i32, vp, fp, fp, fp, fp, vp, vp]),
        "fr_densify_masks": (ci, [i32, fp, fp, fp, i32, f32, f32, f32, vp, vp, vp]),
        "fr_prune_mask": (ci, [i32, fp, fp, i32, f32, f32, vp, vp]),
        "fr_knn_workspace_bytes": (sz, [i32]),
        "fr_knn_dist2": (ci, [i32, fp, fp, vp, sz, vp]),
        "fr_spatial_order_workspace_bytes": (sz, [i32]),
        "fr_spatial_order": (ci, [i32, fp, vp, vp, sz, vp]),
        "fr_profile_enable": (ci, [ci]),
        "fr_profile_fetch": (ci, [P(f32), ci]),
        "fr_occ_workspace_bytes": (sz, [occ]),
        "fr_occ_update": (ci, [occ, fp, i32, i32, i32, P(f32 * 4), P(f32 * 16), P(f32), i32, i32, i32, fp, vp, sz, vp]),
        "fr_occ_freespace": (ci, [occ, fp, fp, i32, vp, vp, sz, vp]),
        "fr_occ_frontiers": (ci, [occ, fp, vp, i32, i32, i32, i32, vp, vp, vp, i32, vp, vp, sz, vp]),
        "fr_occ_erode": (ci, [occ, vp, vp, i32, vp]),
        "fr_occ_cells_of": (ci, [occ, fp, i32, vp, vp]),
        "fr_occ_ring_candidates": (ci, [occ, fp, i32, i32, f32, f32, f32, u32, vp, i32, fp, vp, vp]),
        "fr_occ_free_candidates": (ci, [occ, vp, f32, u32, fp, i32, vp, vp, sz, vp]),
        "fr_plan_workspace_bytes": (sz, [occ]),
        "fr_plan_round_cap": (i32, [occ]),
        "fr_plan_grid": (ci, [occ, fp, fp, i32, f32, i32, i32, vp, vp, vp, sz, vp]),
        "fr_plan_tiers": (ci, [occ, vp, vp, vp]),
        "fr_plan_field": (ci, [occ, vp, i32, i32, vp, vp, P(i32 * 2), vp, sz, vp]),
        "fr_plan_paths": (ci, [occ, vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, vp]),
        "fr_plan_actions": (ci, [occ, vp, i32, vp, vp, vp, i32, P(f64), f64, f64, f64, i32, f64] + [vp] * 7),
        "fr_rollout_actions": (ci, [P(f64), vp, vp, i32, i32, f64, f64, vp, vp, vp]),
        "fr_plan_actions_object": (ci, [occ, vp, i32, vp, vp, vp, i32, P(f64), f64, f64, f64, f64] + [vp] * 9),
        "fr_occ_object_cells": (ci, [occ, vp, i32, i32, vp, i32, vp, vp, sz, vp]),
        "fr_occ_grid_candidates": (ci, [occ, vp, i32, vp, vp, i32, f32, f32, i32, i32, i32, f32, u32, vp, i32, vp, vp, vp]),
        "fr_cloud_index_bytes": (sz, [i32]),
        "fr_cloud_index_workspace_bytes": (sz, [i32]),
        "fr_cloud_query_workspace_bytes": (sz, [i32]),
        "fr_cloud_index_build": (ci, [i32, fp, vp, sz, vp, sz, vp]),
        "fr_cloud_query": (ci, [vp, sz, i32, P(CloudQueryCfg), vp, sz, vp]),
        "fr_dbscan_workspace_bytes": (sz, [i32]),
        "fr_target_select_workspace_bytes": (sz, [i32]),
        "fr_dbscan": (ci, [i32, fp, f32, i32, vp, vp, vp, sz, vp]),
        "fr_target_select": (ci, [i32, fp, fp, f32, f32, f32, f32, i32] + [vp] * 7 + [sz, vp]),
        "fr_view_metrics_workspace_bytes": (sz, [i32] * 3),
        "fr_view_metrics": (ci, [P(ViewMetricsCfg)] + [vp] * 8 + [sz, vp]),
        "fr_view_metrics_summary": (ci, [vp, i32, vp, vp]),
        "fr_loss_mask_workspace_bytes": (sz, [i32] * 2),
        "fr_loss_mask": (ci, [P(LossMaskCfg), fp, fp] + [vp] * 4 + [sz, vp]),
        "fr_bg_penalty_workspace_bytes": (sz, [i32] * 2),
        "fr_bg_penalty_forward": (ci, [i32, i32, f32, f32, fp, fp, vp, fp, fp, vp, sz, vp]),
        "fr_bg_penalty_backward": (ci, [i32, i32, f32, f32, fp, fp, vp, fp, fp, fp, fp, vp]),
        "fr_outside_mask_workspace_bytes": (sz, [i32]),
        "fr_outside_mask": (ci, [i32, i32, fp, fp, fp, fp, vp, i32, i32, vp, vp, vp, sz, vp]),
    }


PROTOTYPES = _prototypes()
EXPORTS = tuple(PROTOTYPES)

_lib = None

_CSRC = os.path.join(os.path.dirname(_HERE), "csrc")
_INCLUDE = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include")


def _in_csrc(*suffixes):
    return sorted(os.path.join(_CSRC, n) for n in os.listdir(_CSRC) if n.endswith(suffixes)) if os.path.isdir(_CSRC) else []


# the manifest: what is in csrc/ IS the library.  UNITS is what build() compiles, SOURCES what the build id is taken over.
UNITS = _in_csrc(".hip")
HEADERS = [os.path.join(_INCLUDE, n) for n in ("fisher_rast.h", "fisher_occ.h")]
SOURCES = UNITS + _in_csrc(".h", ".inc") + HEADERS


def source_hash(files=None):
    """sha256 (first 16 hex digits) over the kernel and header sources (SOURCES, or `files` in their place), or None when they are
    not beside the package."""
    import hashlib
    h = hashlib.sha256()
    for f in (SOURCES if files is None else files):
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
    for name, (restype, argtypes) in PROTOTYPES.items():
        if not hasattr(lib, name):
            if ab_build:
                continue
            raise FisherRastError(f"{SO_PATH} does not export {name}")
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    # a stale or foreign binary must not pass for the sources beside it (FISHER_RAST_SO builds for A/B runs are exempt)
    want = source_hash()
    got = lib.fr_build_id().decode().split(":")[-1]
    if not ab_build and want is not None and got != want:
        raise FisherRastError(f"{SO_PATH} was built from other sources (build id {got}, sources {want}): "
                              "run `python -c \"import __graft_entry__ as g; g.build()\"`")
    _lib = lib
    return lib


def check(rc, what):
    if rc != FR_OK:
        msg = load().fr_last_error().decode("utf-8", "replace")
        raise FisherRastError(f"{what} failed (code {rc}): {msg}")
