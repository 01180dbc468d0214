"""`GaussianSLAM`: the Fisher-information / render operator surface of the reference class
(models/SLAM/gaussian.py) on MI355X.

In scope (same names, arguments and return conventions as the reference):
    compute_Hessian (1503-1570)   compute_H_train (1338-1348)   pose_eval (1354-1375)
    render_at_pose (555-579)      gs_pts_cnt (1350-1352)        gaussian_points / cur_frame_idx (1590-1598)
    render_at_poses (new: render_at_pose for a batch of poses in one call, RenderOps)
    pose_eval_points (new: the candidate scan of global_planning, 1285-1316 -- per-Gaussian scores and their running maximum, PointScoreOps)
    select_target_points / global_planning (1176-1336: the target selection -- height band, quantile, DBSCAN, best cluster -- and the
        planning round assembled on the library, TargetSelectOps; opt-in, not on GaussianSLAM by default)
    pause / resume / color_refinement / stop (1600-1614)
    get_pointcloud / initialize_params / initialize_new_params / add_new_gaussians (75-182, 299-414: module-level functions; the
        frame ingest, FrameIngestOps)
    prune_gaussians / densify / remove_points (models/SLAM/utils/slam_external.py 235-262, 345-463: the map edit, MapEditOps)
    keyframe_selection_overlap (models/SLAM/utils/keyframe_selection.py 40-134: the mapping window, KeyframeSelectOps)
The SLAM loop itself (init, track_rgbd ...) is NOT rebuilt: it is reference
Python that stays as it is.  `FisherOps.install(cls)` grafts the accelerated methods onto the reference class
so that tester_gaussians_navigation.py keeps calling `slam.pose_eval(...)` unchanged; `GaussianSLAM` below is
the same operator surface as a standalone object built from a parameter dict (a `params{t}.npz` checkpoint
or synthetic data) for tests and benchmarks.

What changes underneath: instead of one rasteriser forward + backward(power=2) + cat + sum per view, with
per-view allocations and two host syncs, every call batches its views through FisherScorer
(fisher_rast/ops.py -> fr_fisher_views) and synchronises once when the scores are brought to the host.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from diff_gaussian_rasterization import GaussianRasterizer as Renderer
from fisher_rast import object_loss as _object_loss
from fisher_rast import ops as _ops
from fisher_rast.ops import FisherScorer
from models.SLAM.utils.common_utils import checkpoint_time_idx, load_params_ckpt, save_params, save_params_ckpt
from models.SLAM.utils.recon_helpers import setup_camera
from models.SLAM.utils.slam_helpers import (transformed_params2rendervar, transformed_params2depthplussilhouette,
                                            render_rgb_depth_sil, frame_render_vars)
from models.SLAM.utils.slam_external import update_seen_and_radius, remove_points  # noqa: F401  (remove_points: looked up in this module by global_planning)


def _loss_pixel_mask(depth_sil, gt_depth, sil_thres, reject_outliers, need_presence):
    """Pixels that enter the tracking / mapping loss, from the depth / silhouette / depth^2 render `depth_sil` [3,H,W] -- the rule of
    the reference's get_loss (models/SLAM/gaussian.py:212-233) as one conjunction: a measured depth; with `reject_outliers` an
    absolute depth error below ten times its median (taken over the whole frame: the zeros of unmeasured pixels count, as they do
    there); no NaN in the rendered depth nor in its variance proxy E[z^2] - E[z]^2; with `need_presence` a silhouette above the
    threshold.  Returns (rendered depth [1,H,W], boolean mask [1,H,W])."""
    rendered = depth_sil[0:1]
    keep = gt_depth > 0
    if reject_outliers:
        err = (gt_depth - rendered).abs() * keep
        keep = keep & (err < 10 * err.median())
    keep = keep & ~(torch.isnan(rendered) | torch.isnan(depth_sil[2:3] - rendered ** 2))
    if need_presence:
        keep = keep & (depth_sil[1] > sil_thres)
    return rendered, keep.detach()


def _object_mask_of(curr_data, device):
    """curr_data['obj_mask_2d'] as the object lines of the reference's get_loss take it (models/SLAM/gaussian_object.py:236-242): bool
    [H,W] on the render's device, or None when the frame has none"""
    obj = curr_data.get('obj_mask_2d', None)
    if obj is None:
        return None
    if obj.dtype != torch.bool:
        obj = obj.bool()
    if obj.ndim == 3:
        obj = obj.squeeze(-1)
    return obj.to(device)


def _background_penalty_torch(im, silhouette, obj, lambda_rgb=0.1, lambda_alpha=0.1):
    """The two background penalties of the object class as the reference writes them (models/SLAM/gaussian_object.py:263-275): the
    mean |im| and the mean clamped silhouette over the pixels outside the object mask `obj` (bool [H,W]), weighted -- what is added
    to the colour term."""
    bg1 = (~obj).unsqueeze(0)
    bg3 = torch.tile(bg1, (3, 1, 1)).float()
    l_rgb = (torch.abs(im) * bg3).sum() / bg3.sum().clamp_min(1)
    l_alpha = (silhouette.clamp(min=0, max=1) * bg1).sum() / bg1.sum().clamp_min(1)
    return lambda_rgb * l_rgb + lambda_alpha * l_alpha


def make_get_loss(transform_to_frame, calc_loss, fused_rendervar=False, fused_mask=False, object_mask=False):
    """Drop-in for the module-level `get_loss` of the reference (models/SLAM/gaussian.py:184-297): same signature, same return
    `(loss, variables, weighted_losses)`.  What changes: the two rasteriser calls of 205-211 (RGB, then depth / silhouette /
    depth^2 on the same Gaussians) are ONE projection / binning / sort with two compositing passes and one fused backward
    (`render_rgb_depth_sil` -> fr_forward_pair / fr_backward_pair), and the `seen` / `max_2D_radius` update of 289-291 is one
    kernel pass (fr_densify_stats).  The loss terms are the reference's own `calc_loss` and the pose / point transform its own
    `transform_to_frame` (models/SLAM/utils/slam_helpers.py:23-44, 282-317), handed in by the caller; the pixel mask is
    `_loss_pixel_mask`.  The matplotlib dump of 240-284 is not reproduced (visualize_tracking_loss is accepted and ignored).
    Opt-in: `FisherOps.install(cls, patch_get_loss=True)` puts it into the reference module.  With `fused_rendervar=True` the
    stretch between `params` and the rasteriser -- transform_to_frame, the depth / silhouette features and the activations -- is one
    launch forward and one backward, two with the camera's gradient (`frame_render_vars`, fr_rendervar_forward / _backward), instead
    of the torch chain; a call whose parameters the kernels do not take (not float32, not contiguous, not on one HIP device) goes
    the torch route, that call only.  With `object_mask=True` the step is the object class's (models/SLAM/gaussian_object.py:236-275):
    `curr_data['obj_mask_2d']` is ANDed into the pixel mask and the two background penalties are added to the colour term; a frame
    without one (missing or None) gets neither.  Off by default: without it `obj_mask_2d` is not read.  With `fused_mask=True` the
    pixel mask -- and with `object_mask` the AND and the penalties -- come from the kernels (`fisher_rast.object_loss`: fr_loss_mask,
    fr_bg_penalty_forward / _backward) instead of the torch chain, which stays the route of a call that the kernels do not take."""
    @torch.enable_grad()
    def get_loss(params, curr_data, variables, iter_time_idx, loss_weights, use_sil_for_loss,
                 sil_thres, use_l1, ignore_outlier_depth_loss, tracking=False,
                 mapping=False, do_ba=False, plot_dir=None, visualize_tracking_loss=False, tracking_iteration=None):
        if not (tracking or mapping):
            raise ValueError("get_loss: one of tracking / mapping must be set")     # (the reference fails with a NameError here)
        # tracking: only the camera pose takes a gradient; mapping: only the Gaussians (gaussian.py:189-199)
        rendervar = feats = None
        if fused_rendervar:
            try:
                rendervar, feats = frame_render_vars(params, iter_time_idx, curr_data['w2c'], gaussians_grad=not tracking, camera_grad=bool(tracking))
            except _ops.RenderVarUnsupported:
                pass
        if rendervar is None:
            pts = transform_to_frame(params, iter_time_idx, gaussians_grad=not tracking, camera_grad=bool(tracking))
            im, radius, depth_sil, rendervar = render_rgb_depth_sil(params, curr_data['cam'], curr_data['w2c'], pts)
        else:
            im, radius, depth_sil, rendervar = render_rgb_depth_sil(params, curr_data['cam'], curr_data['w2c'], rendervar['means3D'],
                                                                    rendervar=rendervar, feats=feats)
        variables['means2D'] = rendervar['means2D']      # densification reads the colour render's screen-space gradient (gaussian.py:207)
        need_presence = tracking and use_sil_for_loss
        obj = _object_mask_of(curr_data, depth_sil.device) if object_mask else None
        depth = mask = penalty = None
        if fused_mask:
            try:
                depth, mask = _object_loss.loss_pixel_mask(depth_sil, curr_data['depth'], sil_thres, ignore_outlier_depth_loss, need_presence, obj)
                if obj is not None:
                    penalty = _object_loss.background_penalty(im, depth_sil, obj)
            except _object_loss.ObjectLossUnsupported:
                depth = mask = penalty = None
        if mask is None:
            depth, mask = _loss_pixel_mask(depth_sil, curr_data['depth'], sil_thres, ignore_outlier_depth_loss, need_presence)
            if obj is not None:
                mask = mask & obj.unsqueeze(0)
                penalty = _background_penalty_torch(im, depth_sil[1], obj)
        terms = calc_loss(curr_data, im, depth, mask, mask.repeat(3, 1, 1), use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking)
        if penalty is not None:
            terms['im'] = terms['im'] + penalty
        weighted = {name: value * loss_weights[name] for name, value in terms.items()}
        total = sum(weighted.values())
        update_seen_and_radius(variables, radius)        # variables['seen'], variables['max_2D_radius'] (gaussian.py:289-291)
        weighted['loss'] = total
        return total, variables, weighted
    return get_loss


# ---- frame ingest: new Gaussians from an RGB-D frame (the reference's gaussian.py:75-182, 299-414) ---------------------------------

def _frame_f32(t, name):
    """a frame tensor as the kernels read it: contiguous float32 on its GPU"""
    if not t.is_cuda:
        raise _ops.FisherRastError(f"{name} must live on the GPU (there is no CPU fallback for this path)")
    t = t.detach()
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def get_pointcloud(color, depth, intrinsics, w2c, transform_pts=True, downsample=1,
                   mask=None, compute_mean_sq_dist=False, mean_sq_dist_method="projective"):
    """The reference's get_pointcloud (gaussian.py:75-143), same arguments and returns: the pixels of an RGB-D frame taken at one in
    `downsample`, back-projected -- point_cld [N,6] (xyz + rgb) and, with `compute_mean_sq_dist`, mean3_sq_dist [N].  One launch
    without a mask (no host synchronisation); with one, the mask is max-pooled and compacted on the device and the row count is read
    once (the reference's `sum() > 0`).  Kept from the reference: depth and colour are those of a block's top-left pixel while the
    mask is the block's maximum, and a mask that selects nothing returns every point with a warning.  `downsample` must divide the
    image size (the reference's own shapes disagree otherwise)."""
    if compute_mean_sq_dist and mean_sq_dist_method != "projective":
        raise ValueError(f"Unknown mean_sq_dist_method {mean_sq_dist_method}")
    color, depth = _frame_f32(color, "color"), _frame_f32(depth, "depth")
    H, W = int(color.shape[1]), int(color.shape[2])
    depth = depth.reshape(1, H, W)
    workspace = _ops.frame_ingest_workspace(H, W, downsample, color.device) if mask is not None else None
    count = (H // downsample) * (W // downsample)
    if mask is not None:
        status, _ = _ops.frame_ingest_select(gt_depth=depth, mask=mask.reshape(H, W), downsample=downsample, workspace=workspace)
        selected = int(status[0])                       # the one host read
        if selected > 0:
            count = selected
        else:
            print("[WARN] Mask become all zero after downsampling")
            workspace = None
    point_cld = torch.empty((count, 6), dtype=torch.float32, device=color.device)
    mean3_sq_dist = torch.empty((count,), dtype=torch.float32, device=color.device) if compute_mean_sq_dist else None
    _ops.frame_ingest_emit(color, depth, intrinsics, w2c, workspace, count, downsample=downsample, transform_pts=transform_pts,
                           point_cld=point_cld, mean3_sq_dist=mean3_sq_dist)
    return (point_cld, mean3_sq_dist) if compute_mean_sq_dist else point_cld


def _as_parameters(tensors):
    return {k: torch.nn.Parameter(v.detach().float().contiguous().requires_grad_(True)) for k, v in tensors.items()}


def _gaussian_rows(pt_cld, mean3_sq_dist, isotropic):
    """the five per-Gaussian tensors of a point cloud [N,6]: identity rotations, logit opacity 0, log scale log(sqrt(mean3_sq_dist))"""
    n, dev = int(pt_cld.shape[0]), pt_cld.device
    rots = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    rots[:, 0] = 1.0
    return {
        'means3D': pt_cld[:, :3],
        'rgb_colors': pt_cld[:, 3:6],
        'unnorm_rotations': rots,
        'logit_opacities': torch.zeros((n, 1), dtype=torch.float32, device=dev),
        'log_scales': torch.log(torch.sqrt(mean3_sq_dist))[:, None].repeat(1, 1 if isotropic else 3),
    }


def initialize_params(init_pt_cld, num_frames, mean3_sq_dist, w2c=None, isotropic=False):
    """The reference's initialize_params (gaussian.py:145-182): (params, variables) of a first map -- the Gaussians of a point cloud
    and one camera trajectory of `num_frames` identity poses."""
    dev = init_pt_cld.device
    tensors = _gaussian_rows(init_pt_cld, mean3_sq_dist, isotropic)
    cam_rots = torch.zeros((1, 4, num_frames), dtype=torch.float32, device=dev)
    cam_rots[:, 0] = 1.0
    tensors['cam_unnorm_rots'] = cam_rots
    tensors['cam_trans'] = torch.zeros((1, 3, num_frames), dtype=torch.float32, device=dev)
    params = _as_parameters(tensors)
    n = int(params['means3D'].shape[0])
    variables = {k: torch.zeros(n, dtype=torch.float32, device=dev) for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep')}
    return params, variables


def initialize_new_params(new_pt_cld, mean3_sq_dist, isotropic=False):
    """The reference's initialize_new_params (gaussian.py:299-318)."""
    return _as_parameters(_gaussian_rows(new_pt_cld, mean3_sq_dist, isotropic))


def frame_w2c(params, time_idx):
    """[4,4] world->camera pose of frame `time_idx` from the camera trajectory in `params` (gaussian.py:347-351), on the device"""
    q = F.normalize(params['cam_unnorm_rots'][..., time_idx].detach())[0]
    r, x, y, z = q[0], q[1], q[2], q[3]
    rot = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                       2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                       2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y))).reshape(3, 3)
    w2c = torch.eye(4, dtype=torch.float32, device=rot.device)
    w2c[:3, :3] = rot
    w2c[:3, 3] = params['cam_trans'][..., time_idx].detach()[0]
    return w2c


def _transform_to_frame(params, time_idx, gaussians_grad, camera_grad):
    """The Gaussians' centres in the frame of camera `time_idx`, for the module-level add_new_gaussians (which needs no gradient);
    `FrameIngestOps.install` hands the patched module's own transform_to_frame to `make_add_new_gaussians` instead."""
    pts = params['means3D'].detach()
    w2c = frame_w2c(params, time_idx)
    return pts @ w2c[:3, :3].T + w2c[:3, 3]


def _random_gaussians(params, new_means):
    """gaussian.py:365-397: up to 200 random points in the outer shell of the bounding box of the map and the frame's new points, at
    the robot's height, with random colours and mean3_sq_dist 0.5.  Plain torch, as in the reference (`.item()` and the boolean
    indexing synchronise the host); off in every shipped config.  Returns (point_cld [M,6], mean3_sq_dist [M])."""
    dev = new_means.device
    num_pts = int(min(params["means3D"].shape[0], 1e2))
    hi = torch.maximum(params["means3D"].detach().max(dim=0)[0], new_means.max(dim=0)[0])
    lo = torch.minimum(params["means3D"].detach().min(dim=0)[0], new_means.min(dim=0)[0])
    extent, center = (hi - lo) / 2, (hi + lo) / 2
    center[1] = params["cam_trans"][0, 1, 0].item()
    extent[1] = 1.0
    seed = torch.rand((num_pts * 2, 3), device=dev) * 2 - 1
    inside = (seed[:, 0].abs() <= 0.8) & (seed[:, 2].abs() <= 0.8)
    seed = seed[~inside]
    seed[:, 1] = torch.rand((len(seed),), device=dev) - 0.5
    cld = torch.cat([seed * extent + center, torch.rand((len(seed), 3), device=dev)], dim=-1)
    return cld, torch.ones((len(seed),), device=dev) * .5


def make_add_new_gaussians(transform_to_frame, renderer_cls=None, object_mask=False):
    """Drop-in for the module-level `add_new_gaussians` of the reference (models/SLAM/gaussian.py:320-414): same signature, same
    return `(params, variables)`.  The depth / silhouette render is the caller's (`transform_to_frame` and the rasteriser class are
    handed in, as `make_get_loss` takes its pieces); everything behind it -- depth error, its median, the non-presence mask, the
    max-pool, the selection, the inverse pose, the back-projection and the new parameter rows -- is fr_frame_ingest_select and
    fr_frame_ingest_emit with ONE host read between them (the row count, which sizes the new tensors).  A frame that the map
    explains returns `params` and `variables` as they came.  Otherwise every per-Gaussian parameter is allocated once at its new
    size, the old rows are copied and the kernel writes the new rows in place (no point cloud, no cat of temporaries).
    `add_rand_gaussians` (the signature's default, off in every shipped config) appends the reference's random shell points behind
    the frame's rows in plain torch; it is not accelerated.  The reference's print of the scale range (two more host reads) is left out.
    `object_mask=True` is the function of the object-aware module (models/SLAM/gaussian_object.py:431-525), which differs in one
    step: the non-presence mask is ANDed with `curr_data['obj_mask_2d']` [H,W] before the depth filter (447-460), so new Gaussians
    appear inside the object mask only.  The mask goes to the select kernel as bytes.  (An entry that is missing or None means no
    mask here; the reference fails on it.)"""
    def add_new_gaussians(config, params, variables, curr_data, sil_thres,
                          time_idx, mean_sq_dist_method, densify_dict,
                          add_rand_gaussians=True, downsample_pcd=1):
        if mean_sq_dist_method != "projective":
            raise ValueError(f"Unknown mean_sq_dist_method {mean_sq_dist_method}")
        renderer = renderer_cls or Renderer
        pts = transform_to_frame(params, time_idx, gaussians_grad=False, camera_grad=False)
        rendervar = transformed_params2depthplussilhouette(params, curr_data['w2c'], pts)
        depth_sil, _, _ = renderer(raster_settings=curr_data['cam'])(**rendervar)
        depth_sil, gt_depth = _frame_f32(depth_sil, "the depth / silhouette render"), _frame_f32(curr_data['depth'], "curr_data['depth']")
        obj_mask = curr_data.get('obj_mask_2d', None) if object_mask else None
        status, workspace = _ops.frame_ingest_select(depth_sil, gt_depth, and_mask=obj_mask, downsample=downsample_pcd, sil_thres=sil_thres,
                                                     depth_error_ratio=densify_dict["depth_error_ratio"])
        count = int(status[0])                          # the one host read
        if count == 0:
            return params, variables
        isotropic = bool(config["isotropic"])
        old = {k: params[k].detach() for k in ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales')}
        P, dev = int(old['means3D'].shape[0]), depth_sil.device
        extra = None
        if add_rand_gaussians:
            # the shell needs the frame's new points first: emit them on their own, then lay everything out once
            frame_means = torch.empty((count, 3), dtype=torch.float32, device=dev)
            _ops.frame_ingest_emit(_frame_f32(curr_data['im'], "curr_data['im']"), gt_depth, curr_data['intrinsics'], frame_w2c(params, time_idx),
                                   workspace, count, downsample=downsample_pcd, means3D=frame_means)
            extra = initialize_new_params(*_random_gaussians(params, frame_means), isotropic=isotropic)
        n_extra = 0 if extra is None else int(extra['means3D'].shape[0])
        total = P + count + n_extra
        new = {k: torch.empty((total,) + tuple(v.shape[1:]), dtype=torch.float32, device=dev) for k, v in old.items()}
        if new['log_scales'].shape[1] != (1 if isotropic else 3):
            raise ValueError(f"add_new_gaussians: log_scales has {new['log_scales'].shape[1]} columns, config['isotropic'] is {isotropic}")
        for k, v in old.items():
            new[k][:P] = v
            if extra is not None:
                new[k][P + count:] = extra[k].detach()
        _ops.frame_ingest_emit(_frame_f32(curr_data['im'], "curr_data['im']"), gt_depth, curr_data['intrinsics'], frame_w2c(params, time_idx),
                               workspace, count, downsample=downsample_pcd, row_offset=P, **new)
        for k, v in new.items():
            params[k] = torch.nn.Parameter(v.requires_grad_(True))
        for k in ('means2D_gradient_accum', 'denom', 'max_2D_radius'):
            variables[k] = torch.zeros(total, dtype=torch.float32, device=dev)
        variables['timestep'] = torch.cat((variables['timestep'], torch.full((count + n_extra,), float(time_idx), dtype=torch.float32, device=dev)), dim=0)
        return params, variables
    return add_new_gaussians


add_new_gaussians = make_add_new_gaussians(_transform_to_frame)


class FisherOps:
    """Mixin with the accelerated Fisher methods.  Needs: self.params (dict of tensors), self.cam
    (GaussianRasterizationSettings), self.keyframe_list (dicts with 'est_w2c')."""

    FISHER_COLUMNS = 4       # [camera-frame mean xyz | opacity]
    H_TRAIN_REG = 0.1        # gaussian.py:1357

    # -- internals -----------------------------------------------------------------------------------
    def _device(self):
        return self.params['means3D'].device

    def _as_w2c(self, m):
        if isinstance(m, np.ndarray):
            m = torch.from_numpy(m)
        return m.to(self._device()).float()

    _PARAM_KEYS = ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales')

    def _scorer_key(self, extra):
        """Identity + version of every tensor the scorer is built from: an in-place optimiser step bumps `_version`, a
        densification / pruning pass replaces the tensors -- either way the key changes and the scorer is rebuilt."""
        def sig(t):
            return None if t is None else (id(t), t._version, t.data_ptr(), tuple(t.shape))
        key = [sig(self.params.get(k, None)) for k in self._PARAM_KEYS] + [id(self.cam), self.FISHER_COLUMNS]
        if extra is not None and extra is not False:
            key += [sig(extra[k]) for k in ('means3D', 'rotations', 'opacity', 'scales')]
        return tuple(key)

    def _scorer(self, extra=None):
        """Activated render variables (gaussian.py:1529-1533) wrapped in a FisherScorer, with its packed inputs and workspace.
        Kept between calls while the map is unchanged (the tester scores ~630 path steps per planning round on one map);
        `extra` appends random Gaussians (gaussian_object.py:1971-1992)."""
        key = self._scorer_key(extra)
        cached = getattr(self, "_scorer_cache", None)
        if cached is not None and cached[0] == key:
            return cached[1]
        p = self.params
        with torch.no_grad():
            means = p['means3D'].detach()
            colors = p['rgb_colors'].detach() if p.get('rgb_colors', None) is not None else \
                torch.full_like(means, 0.5)
            rot = F.normalize(p['unnorm_rotations'].detach())
            op = torch.sigmoid(p['logit_opacities'].detach())
            sc = torch.exp(p['log_scales'].detach())
            if sc.shape[-1] == 1:
                sc = torch.tile(sc, (1, 3))
            if extra is not None and extra is not False:
                dev = means.device
                means = torch.cat([means, extra['means3D'].to(dev).float()], dim=0)
                rot = torch.cat([rot, extra['rotations'].to(dev).float()], dim=0)
                op = torch.cat([op, extra['opacity'].to(dev).float().reshape(-1, 1)], dim=0)
                sc = torch.cat([sc, extra['scales'].to(dev).float()], dim=0)
                colors = torch.cat([colors, torch.full((extra['means3D'].shape[0], 3), 0.5, device=dev)], dim=0)
        scorer = FisherScorer(self.cam, means, colors, rot, op, sc, columns=self.FISHER_COLUMNS, dL_dpix=1e-3)
        self._scorer_cache = (key, scorer)
        return scorer

    # -- reference surface ---------------------------------------------------------------------------
    def compute_Hessian(self, rel_w2c, return_points=False, random_gaussian_params=False, return_pose=False):
        """One view's diagonal Fisher proxy (gaussian.py:1503-1570): (N, C) if return_points else flat
        [means(3N) | opacity(N)] -- the reference flattens per block, not per row (1559-1560)."""
        scorer = self._scorer(random_gaussian_params if self.FISHER_COLUMNS == 11 else None)
        w2c = self._as_w2c(rel_w2c).reshape(1, 4, 4)
        N, C = scorer.P, self.FISHER_COLUMNS
        cur_H = torch.zeros((N, C), dtype=torch.float32, device=self._device())
        res = scorer.run(w2c, out_H=cur_H)
        self._last_vis_count = res["vis_count"]
        if not return_points:
            blocks = [cur_H[:, 0:3].reshape(-1), cur_H[:, 3:4].reshape(-1)]
            if C == 11:
                blocks += [cur_H[:, 4:7].reshape(-1), cur_H[:, 7:11].reshape(-1)]
            cur_H = torch.cat(blocks)
        if not return_pose:
            return cur_H
        pose_H = torch.eye(6, device=self._device())
        if C == 11:
            return cur_H, pose_H, int(self._last_vis_count[0].item())
        return cur_H, pose_H

    def compute_H_train(self, random_gaussians=None):
        """Sum of cur_H over the keyframes (gaussian.py:1338-1348), all keyframes in one batched call."""
        if len(self.keyframe_list) == 0:
            return None
        scorer = self._scorer(random_gaussians if self.FISHER_COLUMNS == 11 else None)   # shared with pose_eval's scoring launch
        w2cs = self._stack_poses([kf['est_w2c'] for kf in self.keyframe_list])
        H_train = torch.zeros((scorer.P, self.FISHER_COLUMNS), dtype=torch.float32, device=self._device())
        scorer.run(w2cs, out_H=H_train)
        return H_train

    def _keyframe_key(self):
        """The keyframe poses as (tensor objects, their versions), or None when they cannot be followed (not device tensors).  The
        cache holds on to the tensor OBJECTS, so a later tensor cannot take a freed one's identity."""
        if not getattr(self, "CACHE_H_TRAIN", True):
            return None
        ts = [kf['est_w2c'] for kf in self.keyframe_list]
        if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
            return None
        return ts, tuple(t._version for t in ts)

    @staticmethod
    def _same_keyframes(a, b):
        return a is not None and b is not None and len(a[0]) == len(b[0]) and a[1] == b[1] and all(x is y for x, y in zip(a[0], b[0]))

    def gs_pts_cnt(self, random_gaussian_params=None):
        """ API Setting """
        return 1

    def _stack_poses(self, poses):
        """[V,4,4] fp32 on the device from a tensor, an array, or a list of either: one stack and one transfer, not V of them"""
        dev = self._device()
        if isinstance(poses, torch.Tensor):
            return poses.reshape(-1, 4, 4).to(dev).float()
        if isinstance(poses, np.ndarray):
            return torch.from_numpy(np.ascontiguousarray(poses.reshape(-1, 4, 4))).to(dev).float()
        if len(poses) and all(isinstance(p, torch.Tensor) and p.device == dev for p in poses):
            return torch.stack(list(poses)).float()
        return torch.from_numpy(np.stack([np.asarray(p.detach().cpu() if isinstance(p, torch.Tensor) else p) for p in poses])).to(dev).float()

    def pose_eval(self, poses, random_gaussian_params=None, criterion=None):
        """Scores of candidate poses (gaussian.py:1354-1375): returns (scores cpu fp32 [V], stack(c2w) [V,4,4]).
        H_train over the keyframes and the candidate scores are two launches on one stream with ONE host synchronisation:
        the two 16-byte status words travel to the host together with the scores."""
        extra = random_gaussian_params if self.FISHER_COLUMNS == 11 else None
        c2w = self._stack_poses(poses)
        scorer = self._scorer(extra)
        V, K = int(c2w.shape[0]), len(self.keyframe_list)
        if 0 < K and max(V, K) <= scorer.max_views_per_launch():
            # H_train is a function of (map, keyframe poses): a planner calls pose_eval for batch after batch of candidates between two
            # mapping steps, so 1 / (H_train + reg) is kept while neither has changed (the scorer is per map version already; the
            # keyframe poses are followed by tensor identity + version -- poses that are not device tensors are not followed, no reuse)
            kkey = self._keyframe_key()
            cached = getattr(self, "_h_inv_cache", None)
            if cached is not None and cached[0] is scorer and self._same_keyframes(cached[1], kkey):
                r2 = scorer.launch(c2w, H_inv=cached[2], poses_are_c2w=True)
                host = torch.cat([r2["status"], r2["scores"].view(torch.int32)]).cpu()
                if int(host[1]) == 0:
                    return host[4:].view(torch.float32).clone(), c2w
            else:
                kf = self._stack_poses([kf['est_w2c'] for kf in self.keyframe_list])
                H_train = torch.zeros((scorer.P, self.FISHER_COLUMNS), dtype=torch.float32, device=self._device())
                r1 = scorer.launch(kf, out_H=H_train)
                # (the poses go in as they are: the library inverts them -- one kernel in place of torch.linalg.inv's dozen launches)
                H_inv = torch.reciprocal(H_train + self.H_TRAIN_REG)
                r2 = scorer.launch(c2w, H_inv=H_inv, poses_are_c2w=True)
                host = torch.cat([r1["status"], r2["status"], r2["scores"].view(torch.int32)]).cpu()      # the one sync
                if int(host[1]) == 0 and int(host[5]) == 0:
                    self._h_inv_cache = (scorer, kkey, H_inv) if kkey is not None else None
                    return host[8:].view(torch.float32).clone(), c2w
            self._h_inv_cache = None
            # the tile-instance buffer was too small (nothing was accumulated or scored): the growing path below repeats both
        H_train = self.compute_H_train(extra)
        H_train_inv = torch.reciprocal(H_train + self.H_TRAIN_REG)
        res = scorer.run(c2w, H_inv=H_train_inv, poses_are_c2w=True)
        scores = res["scores"].cpu()
        return scores, c2w

    def path_scores(self, w2cs, H_inv_per_view):
        """Batched form of the planner's per-step `sum(cur_H * H_train_inv_path)` (tester 1688-1695): every view
        gets its own weight block.  Returns the V sums on the device (the caller takes the log)."""
        scorer = self._scorer()
        return scorer.run(self._as_w2c(w2cs), H_inv=H_inv_per_view, H_inv_per_view=True)["scores"]

    @classmethod
    def install(cls, target_cls, patch_get_loss=False, fused_loss=False, fused_rendervar=False, fused_mask=False, object_mask=False):
        """Graft the accelerated methods onto the reference's class.  `patch_get_loss=True` also replaces the
        module-level `get_loss` of the module `target_cls` lives in by the fused-render form (`make_get_loss`); off by default --
        a caller that only wants the Fisher scorer keeps the reference's training step untouched.  With `fused_loss=True` as well,
        that get_loss takes its loss terms from this package's `calc_loss` (`calc_loss_mask` where the module has one: the object
        class) -- the fused L1 + SSIM kernels, no host synchronisation -- instead of the reference module's own; off by default.  With `fused_rendervar=True`
        as well, it builds the render variables with the fused kernels (`make_get_loss(..., fused_rendervar=True)`); off by default.
        `object_mask=True` makes that get_loss the object class's -- `curr_data['obj_mask_2d']` in the pixel mask, the two background
        penalties in the colour term -- and `fused_mask=True` takes the pixel mask (and the object lines) from the kernels
        (`make_get_loss(..., fused_mask=True, object_mask=True)`); both off by default, also for the object class."""
        for name in ("_device", "_as_w2c", "_stack_poses", "_scorer", "_scorer_key", "_keyframe_key", "_same_keyframes", "_PARAM_KEYS", "compute_Hessian", "compute_H_train",
                     "pose_eval", "path_scores"):
            setattr(target_cls, name, getattr(cls, name))
        # the module-level get_loss of the reference (gaussian.py:184-297), rebuilt around the reference module's own
        # transform_to_frame / calc_loss: one fused render pair instead of two rasteriser calls
        import sys
        mod = sys.modules.get(target_cls.__module__)
        if patch_get_loss and mod is not None and all(hasattr(mod, n) for n in ("get_loss", "transform_to_frame", "calc_loss")):
            loss_fn = mod.calc_loss
            if fused_loss:
                from models.SLAM.utils import slam_helpers as _sh
                loss_fn = _sh.calc_loss_mask if hasattr(mod, "calc_loss_mask") else _sh.calc_loss
            # the keyword only when it is set: a make_get_loss wrapped by a caller with the two-argument signature keeps working
            flags = dict(fused_rendervar=fused_rendervar, fused_mask=fused_mask, object_mask=object_mask)
            mod.get_loss = make_get_loss(mod.transform_to_frame, loss_fn, **{k: True for k, v in flags.items() if v})
        if not hasattr(target_cls, "FISHER_COLUMNS"):
            target_cls.FISHER_COLUMNS = cls.FISHER_COLUMNS
        target_cls.H_TRAIN_REG = cls.H_TRAIN_REG
        return target_cls


class PoseFisherOps:
    """Mixin with the camera-pose Fisher information of candidate views (fr_fisher_pose_views, include/fisher_rast.h): the 6 x 6
    matrix the reference's path objective takes the log-determinant of (tester_gaussians_navigation.py:1689-1701), which its
    compute_Hessian(return_pose=True) returns as eye(6).  That method keeps doing so; these are new names.  xi = (translation,
    rotation), left perturbation of the camera-frame means.  Needs FisherOps' `_scorer` / `_as_w2c` (install FisherOps first)."""

    def compute_pose_Hessian(self, rel_w2c):
        """[6, 6] pose Fisher information of one world->camera pose."""
        return self.pose_Hessians(self._as_w2c(rel_w2c).reshape(1, 4, 4))[0]

    def pose_Hessians(self, w2cs):
        """[V, 6, 6] for V world->camera poses, batched through the scorer of the current map."""
        return self._scorer().pose_fisher(self._as_w2c(w2cs).reshape(-1, 4, 4))

    @classmethod
    def install(cls, target_cls):
        """Graft the two methods onto the reference's class (after FisherOps.install / ObjectFisherOps.install)."""
        for name in ("compute_pose_Hessian", "pose_Hessians"):
            setattr(target_cls, name, getattr(cls, name))
        return target_cls


class RenderOps:
    """Mixin with the batched render of candidate poses (fr_render_views, include/fisher_rast.h): `render_at_pose` for V poses in one
    call -- the reference renders every candidate it scores, one pose at a time (models/SLAM/gaussian_object.py:1640, 1668).
    `render_at_pose` itself stays as it is; this is a new name.  Needs FisherOps' `_scorer` / `_stack_poses` (install FisherOps first)."""

    def render_at_poses(self, c2ws):
        """{"render": [V,3,H,W], "depth": [V,1,H,W], "silhouette": [V,1,H,W]} for V camera-to-world poses (tensor, array or list),
        batched through the scorer of the current map.  Per pose: the RGB render, and channels 0 / 1 of the (z, 1, z z) render over
        the camera-frame means -- depth and silhouette (1 - silhouette = how much of the view the map does not explain).  The
        library inverts the poses; the camera-frame means are formed in the fixed order DESIGN.md section 2 states.
        The depth is the camera-frame z of the pose: `render_at_pose` takes it through `self.first_frame_w2c`, which is the identity
        in this product (GaussianSLAM.__init__); on a class whose first frame is not the identity the two "depth" images differ."""
        res = self._scorer().render_views(self._stack_poses(c2ws), poses_are_c2w=True, depth=False, final_T=False)
        depth_sil = res["depth_sil"]
        return {"render": res["render"], "depth": depth_sil[:, 0:1], "silhouette": depth_sil[:, 1:2]}

    def render_views(self, w2cs, features=True, depth=True, final_T=True):
        """The full result of FisherScorer.render_views for V world->camera poses: render [V,3,H,W], depth_sil [V,3,H,W] (z, 1, z z),
        median_depth [V,1,H,W], final_T [V,H,W], vis_count [V], num_rendered [V] (the optional ones None when switched off)."""
        return self._scorer().render_views(self._stack_poses(w2cs), features=features, depth=depth, final_T=final_T)

    @classmethod
    def install(cls, target_cls):
        """Graft the two methods onto the reference's class (after FisherOps.install / ObjectFisherOps.install)."""
        for name in ("render_at_poses", "render_views"):
            setattr(target_cls, name, getattr(cls, name))
        return target_cls


class RenderEvalOps:
    """Mixin with the render-quality evaluation (fr_view_metrics, include/fisher_rast.h; fisher_rast/render_eval.py): the metric loop
    of NavTester.eval_navigation (tester_gaussians_navigation.py:1397-1491) over a batch of poses, and report_progress's metrics of
    one training frame (models/SLAM/utils/eval_helpers.py:230-257).  New names; `render_at_pose` stays as it is.  Needs FisherOps'
    `_scorer` / `_stack_poses` and RenderOps (install them first)."""

    def eval_views(self, c2ws, rgb_gt, depth_gt=None, chunk=64, on_chunk=None):
        """PSNR, SSIM and depth error of V camera-to-world poses against Habitat's images -- rgb_gt uint8 [V,H,W,3|4] (observations['rgb']
        stacked) or float32 [V,3,H,W], depth_gt float32 [V,1,H,W] / [V,H,W] or None -- rendered and scored `chunk` poses at a time with
        one host read.  Returns a fisher_rast.render_eval.ViewEvaluation: .psnr / .ssim / .depth_mae / .depth_rmse / .kept per view and
        .mean, the tester's test/psnr, test/ssim, test/depth_mae (views with an infinite PSNR left out, as there).
        `on_chunk(v0, v1, render, depth)` sees each chunk's clamped images (LPIPS, image dumps)."""
        from fisher_rast.render_eval import evaluate_views
        return evaluate_views(self, c2ws, rgb_gt, depth_gt, chunk=chunk, on_chunk=on_chunk)

    def frame_metrics(self, im, gt_im, depth=None, gt_depth=None, mask=None):
        """report_progress's metrics of one frame on the device, without a host read: {"psnr", "ssim", "depth_l1", "depth_rmse"} as
        0-dim tensors and "row", the frame's 8 floats.  im, gt_im: float32 [3,H,W]; depth, gt_depth: [1,H,W] or [H,W]; mask: the
        presence mask [H,W] / [1,H,W] of the tracking form, which multiplies both images and the depth difference.  No clamp; the
        depth terms run over the pixels with gt_depth > 0.  depth_rmse is sqrt(mean of squares), not the reference's second L1."""
        from fisher_rast.ops import view_metrics

        def one(t):
            return None if t is None else t.reshape((1,) + tuple(t.shape[-2:]))
        r = view_metrics(im.unsqueeze(0), gt_im.unsqueeze(0), one(depth), one(gt_depth), one(mask), clamp=False, depth_valid_only=True)
        row = r["rows"][0]
        return {"psnr": row[0], "ssim": row[1], "depth_l1": row[2], "depth_rmse": row[3], "row": row}

    @classmethod
    def install(cls, target_cls):
        """Graft the two methods onto the reference's class (after FisherOps.install and RenderOps.install)."""
        for name in ("eval_views", "frame_metrics"):
            setattr(target_cls, name, getattr(cls, name))
        return target_cls


class PointScoreOps:
    """Mixin with the per-Gaussian scores of candidate poses (fr_fisher_point_views, include/fisher_rast.h): the candidate scan of
    the reference's `global_planning` (models/SLAM/gaussian.py:1285-1316) -- `pointScores = sum(cur_H * H_train_inv, dim=1)` per
    candidate and the running `max_points_score` that `prune_invisible` reads -- in one batched call, without a [V, P, columns]
    tensor.  `pose_eval` itself stays as it is; this is a new name.  Needs FisherOps' `_scorer` / `_stack_poses` / `compute_H_train`
    (install FisherOps first)."""

    def pose_eval_points(self, poses, random_gaussian_params=None, per_view=False):
        """(scores cpu fp32 [V], stack(c2w) [V,4,4], max_points_score [P] on the device[, point_scores [V,P] with `per_view`]) for
        V camera-to-world poses (tensor, array or list).  scores are `pose_eval`'s (the sum over the Gaussians of a view's point
        scores), with the same 1 / (H_train + H_TRAIN_REG) -- the one `pose_eval` keeps while map and keyframes are unchanged is
        used when it is there.  max_points_score starts from zeros, as the reference's does.  Habitat's navigability filter of the
        reference loop stays the caller's: pass the poses that survive it."""
        extra = random_gaussian_params if self.FISHER_COLUMNS == 11 else None
        c2w = self._stack_poses(poses)
        scorer = self._scorer(extra)
        cached = getattr(self, "_h_inv_cache", None)
        if cached is not None and cached[0] is scorer and self._same_keyframes(cached[1], self._keyframe_key()):
            H_inv = cached[2]
        else:
            H_inv = torch.reciprocal(self.compute_H_train(extra) + self.H_TRAIN_REG)
        res = scorer.point_scores(c2w, H_inv, per_view=per_view, poses_are_c2w=True)
        out = (res["scores"].cpu(), c2w, res["point_max"])
        return out + (res["point_scores"],) if per_view else out

    @classmethod
    def install(cls, target_cls):
        """Graft the method onto the reference's class (after FisherOps.install / ObjectFisherOps.install)."""
        for name in ("pose_eval_points",):
            setattr(target_cls, name, getattr(cls, name))
        return target_cls


class TargetSelectOps:
    """Mixin with the target selection of the reference's `global_planning` (fr_target_select, include/fisher_rast.h) and the
    planning round assembled around it: `install(target_cls)` adds `select_target_points` -- models/SLAM/gaussian.py:1218-1276, the
    same lines at gaussian_object.py:1419-1479 -- and replaces `global_planning` (1176-1336) by one that runs every stage on the
    library: `compute_H_train`, `select_target_points`, one `pose_eval_points` over the poses that survive Habitat's navigability
    filter, and the patched module's `remove_points`.  The class keeps its own `build_frontiers`, `generate_Gaussian_at_frontier`
    and `generate_candidate`.  Needs FisherOps and PointScoreOps installed.  Opt-in: nothing is installed by default.

    What differs from the reference is listed in INTEGRATION.md section 4: binary32 distances in DBSCAN, a non-finite centre is
    noise, the `global_planning_iter{frame}.npz` dump only with `dump_labels=True`, the candidates scored in one batch after the
    navigability loop instead of one by one inside it, no print of the pruned count and no empty_cache()."""

    QUANTILE, DBSCAN_EPS, DBSCAN_MIN_SAMPLES = 0.8, 0.1, 5        # gaussian.py:1226, 1239

    def select_target_points(self, scorePoints, K, dump_labels=False):
        """(center_point [K,3], or [1,3] when nothing is above the threshold, on the device; selected_points_index int64 or None).
        Draws np.random.randint(0, n_selected, (K,)) exactly as gaussian.py:1269 does, so a seeded run draws the same rows; the
        centres are gathered on the device.  When no cluster qualifies, max_label stays -1 and the draw is among the NOISE rows,
        as `labels == max_count_label` selects them there; with no such row np.random.randint raises, as it does there."""
        from fisher_rast.cluster import select_target
        height_range = self.config["explore"]["height_range"]
        lower_y, upper_y = self.cam_height - height_range, self.cam_height + height_range
        means = self.params["means3D"].detach()
        sel = select_target(means, scorePoints.detach(), lower_y, upper_y, q=self.QUANTILE, eps=self.DBSCAN_EPS,
                            min_samples=self.DBSCAN_MIN_SAMPLES)
        self._last_target_selection = sel
        if sel.n_above == 0:
            return means[sel.argmax].unsqueeze(0), None                                       # gaussian.py:1274-1276
        if dump_labels:
            # the reference's dump (1259-1264), the only path that copies labels to the host
            segmentated_labels = np.ones((int(scorePoints.shape[0]),)) * -1
            segmentated_labels[sel.points_index.cpu().numpy()] = sel.labels.cpu().numpy()
            points_index_range_np = sel.points_index_range.cpu().numpy().astype(np.int64)
            np.savez(os.path.join(self.eval_dir, f"global_planning_iter{self.frame_idx}.npz"),
                     segmentated_labels=segmentated_labels[points_index_range_np], max_label=sel.max_label,
                     points_index_range=points_index_range_np)
        selected_points_index = sel.selected_points_index.long()
        draws = np.random.randint(0, sel.n_selected, (K,))
        center_point = means[selected_points_index[torch.from_numpy(draws).to(means.device)]]
        return center_point, selected_points_index

    def global_planning(self, follower, agent_pose):
        """The reference's global_planning (gaussian.py:1176-1336): same arguments, returns (scores cpu [V'], stack of the navigable
        c2w [V',4,4]) or (None, None) when no candidate is navigable."""
        import sys
        for name in ("compute_H_train", "pose_eval_points", "_scorer", "_keyframe_key"):
            if not hasattr(self, name):
                raise RuntimeError(f"TargetSelectOps.global_planning needs FisherOps and PointScoreOps installed on {type(self).__name__} ({name} is missing)")
        # the module whose remove_points MapEditOps.install replaces: that of the class, or of the base a subclass took it from
        mod = next((m for m in (sys.modules.get(c.__module__) for c in type(self).__mro__) if m is not None and hasattr(m, "remove_points")), None)
        frontier = self.build_frontiers()
        self.generate_Gaussian_at_frontier()
        use_frontier = frontier is not None and self.selection < 2

        agent_pos = agent_pose[:3, 3]
        H_train = self.compute_H_train()
        if H_train is None:
            raise RuntimeError("global_planning: no keyframe to take H_train from")
        H_train_inv = torch.reciprocal(H_train + self.H_TRAIN_REG)
        scorePoints = torch.sum(H_train_inv, dim=1)
        kkey = self._keyframe_key()
        if kkey is not None:
            self._h_inv_cache = (self._scorer(None), kkey, H_train_inv)                      # pose_eval_points below reuses it

        with torch.no_grad():
            K = self.config["explore"]["sample_view_num"]
            dev = scorePoints.device
            if use_frontier:
                frontier_height = np.ones((frontier.shape[0], )) * self.cam_height
                frontier = np.stack([frontier[:, 0], frontier_height, frontier[:, 1]], axis=1)
                frontier = torch.from_numpy(frontier).to(dev)
                frontier_rand_index = torch.randint(0, frontier.shape[0], (K, ))
                center_point = frontier[frontier_rand_index.to(dev)]
                selected_points_index = None
            else:
                center_point, selected_points_index = self.select_target_points(scorePoints, K)

            c2ws = self.generate_candidate(center_point)
            positions = torch.stack([c2w[:3, 3] for c2w in c2ws]).cpu().numpy() if len(c2ws) else np.zeros((0, 3))
            navigable_c2w = []
            for c2w, target_pos in zip(c2ws, positions):
                target_pos = target_pos.copy()
                target_pos[1] = agent_pos[1]
                if follower.pathfinder.is_navigable(target_pos):
                    try:
                        follower.reset()
                        len(list(follower.find_path(target_pos)))
                    except Exception:
                        # Some time the follower throws an exception even if it's navigable
                        print(f"[WARN] Exception found when finding action lens for {target_pos}")
                        continue
                    navigable_c2w.append(c2w)

            scores = None
            max_points_score = torch.zeros((scorePoints.shape[0], ), device=dev)
            if len(navigable_c2w):
                scores, navigable_c2w, max_points_score = self.pose_eval_points(navigable_c2w)

            # culling invisible
            if self.config["explore"]["prune_invisible"] and selected_points_index is not None:
                if mod is None:
                    raise RuntimeError(f"global_planning: the module of {type(self).__name__} does not define remove_points")
                low = max_points_score[selected_points_index] < scorePoints[selected_points_index] * 2
                remove_index = torch.zeros((self.params["means3D"].shape[0], ), dtype=torch.bool, device=dev)
                remove_index[selected_points_index] = low
                self.params, self.variables = mod.remove_points(remove_index, self.params, self.variables, None)

            self.selection += 1
            if scores is None:
                return None, None
            return scores, navigable_c2w

    @classmethod
    def install(cls, target_cls):
        """Graft the two methods onto the reference's class (after FisherOps.install and PointScoreOps.install)."""
        for name in ("QUANTILE", "DBSCAN_EPS", "DBSCAN_MIN_SAMPLES", "select_target_points", "global_planning"):
            setattr(target_cls, name, getattr(cls, name))
        return target_cls


class FrameIngestOps:
    """The frame ingest of the mapping loop (fr_frame_ingest_select / fr_frame_ingest_emit, include/fisher_rast.h) for the reference's
    modules: `install(target_cls)` replaces the four module-level functions `get_pointcloud`, `initialize_params`,
    `initialize_new_params` and `add_new_gaussians` of the module `target_cls` lives in (models/SLAM/gaussian.py for GaussianSLAM,
    models/SLAM/gaussian_object.py for GaussianObjectSLAM -- their `init` and `track_rgbd` look these names up in the module), and
    nothing on the class itself.  `add_new_gaussians` renders with that module's own `transform_to_frame` and `Renderer`, and keeps
    the one difference between the two modules' functions: the object module's ANDs `curr_data['obj_mask_2d']` into the mask."""

    INGEST_NAMES = ("get_pointcloud", "initialize_params", "initialize_new_params", "add_new_gaussians")

    @staticmethod
    def _reads_object_mask(fn):
        """whether a module's add_new_gaussians looks at curr_data['obj_mask_2d'] (gaussian_object.py's does, gaussian.py's does not)"""
        if hasattr(fn, "object_mask"):                  # one of ours, installed before
            return bool(fn.object_mask)
        code = getattr(fn, "__code__", None)
        return code is not None and "obj_mask_2d" in code.co_consts

    @classmethod
    def install(cls, target_cls, object_mask=None):
        """`object_mask`: whether the installed add_new_gaussians ANDs `curr_data['obj_mask_2d']` into the non-presence mask, as the
        object-aware module's own function does.  None (default) follows the function being replaced: on when it reads that entry."""
        import sys
        mod = sys.modules.get(target_cls.__module__)
        if mod is None or not all(hasattr(mod, n) for n in cls.INGEST_NAMES + ("transform_to_frame",)):
            raise ValueError(f"FrameIngestOps.install: the module of {target_cls.__name__} does not define {cls.INGEST_NAMES} and transform_to_frame")
        if object_mask is None:
            object_mask = cls._reads_object_mask(mod.add_new_gaussians)
        mod.get_pointcloud = get_pointcloud
        mod.initialize_params = initialize_params
        mod.initialize_new_params = initialize_new_params
        mod.add_new_gaussians = make_add_new_gaussians(mod.transform_to_frame, getattr(mod, "Renderer", None), object_mask=bool(object_mask))
        mod.add_new_gaussians.object_mask = bool(object_mask)
        return target_cls


class MapEditOps:
    """The map edit of the mapping loop (fr_map_edit_plan / fr_map_edit_apply / fr_map_edit_split_children, include/fisher_rast.h)
    for the reference's modules: `install(target_cls)` replaces the module-level functions `prune_gaussians`, `densify` and
    `remove_points` of the module `target_cls` lives in (their `track_rgbd` and `prune_invisible` look these names up in the module),
    and nothing on the class itself.  The object-aware branch of `prune_gaussians` asks that module's own
    `get_gaussians_outside_mask` for the outside mask; with `outside_mask="library"` this package's
    (models/SLAM/utils/slam_external.py: fr_outside_mask, one host read) instead.  Opt-in: nothing is installed by default."""

    EDIT_NAMES = ("prune_gaussians", "densify", "remove_points")

    @classmethod
    def install(cls, target_cls, outside_mask="module"):
        import sys
        from models.SLAM.utils import slam_external as se
        mod = sys.modules.get(target_cls.__module__)
        if mod is None or not all(hasattr(mod, n) for n in cls.EDIT_NAMES):
            raise ValueError(f"MapEditOps.install: the module of {target_cls.__name__} does not define {cls.EDIT_NAMES}")
        if outside_mask not in ("module", "library"):
            raise ValueError(f"MapEditOps.install: outside_mask is 'module' or 'library' (got {outside_mask!r})")
        outside_fn = se.get_gaussians_outside_mask if outside_mask == "library" else getattr(mod, "get_gaussians_outside_mask", None)
        edit = se.MapEdit(se.HipMapEditBackend(), outside_mask_fn=outside_fn)
        mod.prune_gaussians = edit.prune_gaussians
        mod.densify = edit.densify
        mod.remove_points = edit.remove_points
        return target_cls


class KeyframeSelectOps:
    """The keyframe selection of the mapping loop (fr_keyframe_valid_pixels / fr_keyframe_overlap, include/fisher_rast.h) for the
    reference's modules: `install(target_cls)` replaces the module-level name `keyframe_selection_overlap` of the module `target_cls`
    lives in (models/SLAM/gaussian.py and models/SLAM/gaussian_object.py import it by name, and their `track_rgbd` looks it up there
    every `map_every` frames), and nothing on the class itself.  Opt-in: nothing is installed by default."""

    NAME = "keyframe_selection_overlap"

    @classmethod
    def install(cls, target_cls):
        import sys
        from models.SLAM.utils.keyframe_selection import keyframe_selection_overlap
        mod = sys.modules.get(target_cls.__module__)
        if mod is None or not hasattr(mod, cls.NAME):
            raise ValueError(f"KeyframeSelectOps.install: the module of {target_cls.__name__} does not define {cls.NAME}")
        setattr(mod, cls.NAME, keyframe_selection_overlap)
        return target_cls


class OptimizerOps:
    """The optimizer step of the tracking and mapping loops (fr_adam_step, include/fisher_rast.h) for the reference's classes:
    `install(target_cls)` replaces the method `get_optimizer(self, tracking)` (models/SLAM/gaussian.py:1458-1469 and
    models/SLAM/gaussian_object.py:1815-1826, which are identical) by one that builds the same seven groups of one tensor, with the
    same names, learning rates (`self.config[...]["lrs"]`) and eps, and returns a fisher_rast.optim.FusedAdam.  `skip_frozen=True`
    additionally leaves the lr == 0 groups -- the whole map, in tracking -- out of the step (see FusedAdam for what that changes).
    Opt-in: nothing is installed by default."""

    @classmethod
    def install(cls, target_cls, skip_frozen=False):
        from fisher_rast.optim import FusedAdam

        def get_optimizer(self, tracking):
            lrs_dict = self.config["tracking"]["lrs"] if tracking else self.config["mapping"]["lrs"]
            param_groups = [{'params': [v], 'name': k, 'lr': lrs_dict[k]} for k, v in self.params.items()]
            if tracking:
                return FusedAdam(param_groups, skip_frozen=skip_frozen)
            return FusedAdam(param_groups, lr=0.0, eps=1e-15, skip_frozen=skip_frozen)

        target_cls.get_optimizer = get_optimizer
        return target_cls


class GaussianSLAM(FisherOps, PoseFisherOps, RenderOps, RenderEvalOps, PointScoreOps):
    """Standalone carrier of the operator surface: a Gaussian map (param dict), a camera and keyframes."""

    def __init__(self, config=None, params=None, intrinsics=None, width=None, height=None, device="cuda"):
        self.config = config
        self.cfg = config
        if config is not None and intrinsics is None:
            cal = config["SLAM"]["Dataset"]["Calibration"] if "SLAM" in config else config["Dataset"]["Calibration"]
            intrinsics = np.array([[cal["fx"], 0.0, cal["cx"]], [0.0, cal["fy"], cal["cy"]], [0.0, 0.0, 1.0]])
            width = width or cal.get("width", None)
            height = height or cal.get("height", None)
        self.device = torch.device(device)
        self.intrinsics = None if intrinsics is None else torch.as_tensor(np.asarray(intrinsics)).float().to(self.device)
        self.params = {}
        self.variables = {}
        self.checkpoint_extras = {}
        self.cam = None
        self.frame_idx = 0
        self.keyframe_list = []
        self.keyframe_time_indices = []
        self.first_frame_w2c = torch.eye(4, device=self.device)
        self.save_dir = self.eval_dir = None
        if params is not None:
            self.load_params(params)
        if intrinsics is not None and width is not None and height is not None:
            self.set_camera(width, height, intrinsics)

    # -- construction helpers (checkpoint format: common_utils.py:45-59, gaussian.py:156-168) ----------
    def load_params(self, params):
        """`params`: a dict of arrays / tensors, or the path of a `params{t}.npz` / `params.npz` checkpoint written by the
        reference (common_utils.py:35-59).  A path is read the way tester_gaussians_navigation.py:2745-2760 does: the extras
        "Uncertainty" / "occ_map" are kept aside, the densification statistics are reset, and
        `keyframe_time_indices{t}.npy` next to `eval_dir` is picked up when it exists."""
        if isinstance(params, (str, os.PathLike)):
            weight_file = os.fspath(params)
            self.params, self.checkpoint_extras = load_params_ckpt(weight_file, device=self.device)
            n = self.params['means3D'].shape[0]
            for k in ('max_2D_radius', 'means2D_gradient_accum', 'denom', 'timestep'):
                self.variables[k] = torch.zeros(n, device=self.device, dtype=torch.float32)
            t = checkpoint_time_idx(weight_file)
            if t is not None:
                self.frame_idx = t
                kf_file = os.path.join(self.eval_dir or os.path.dirname(weight_file), f"keyframe_time_indices{t}.npy")
                if os.path.exists(kf_file):
                    self.keyframe_time_indices = np.load(kf_file).tolist()
            return self
        self.params = {k: torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).float().to(self.device)
                       for k, v in params.items()}
        return self

    def save_params_ckpt(self, output_dir, time_idx=None, **extra_args):
        """Writes `params{time_idx}.npz` (or `params.npz`) in the reference's format."""
        if time_idx is None:
            return save_params(self.params, output_dir)
        return save_params_ckpt(self.params, output_dir, time_idx, **extra_args)

    def set_camera(self, width, height, intrinsics):
        k = np.asarray(intrinsics.cpu() if isinstance(intrinsics, torch.Tensor) else intrinsics)
        self.intrinsics = torch.as_tensor(k).float().to(self.device)
        # the view matrix is identity: Gaussians are moved into the candidate frame instead (gaussian.py:493-495)
        self.cam = setup_camera(width, height, k, np.eye(4), device=self.device)
        return self

    def add_keyframe(self, est_w2c, **extra):
        kf = dict(est_w2c=self._as_w2c(est_w2c), id=len(self.keyframe_list))
        kf.update(extra)
        self.keyframe_list.append(kf)
        return kf

    # -- rendering (gaussian.py:555-579) ---------------------------------------------------------------
    def render_at_pose(self, c2w, white_bg=True, mask=None):
        rel_w2c = torch.linalg.inv(self._as_w2c(c2w))
        pts = self.params['means3D']
        pts4 = torch.cat((pts, torch.ones_like(pts[:, :1])), dim=1)
        transformed_pts = (rel_w2c @ pts4.T).T[:, :3]
        rendervar = transformed_params2rendervar(self.params, transformed_pts)
        depth_sil_rendervar = transformed_params2depthplussilhouette(self.params, self.first_frame_w2c, transformed_pts)
        im, radius, _, = Renderer(raster_settings=self.cam)(**rendervar)
        self.variables['means2D'] = rendervar['means2D']
        depth_sil, _, _, = Renderer(raster_settings=self.cam)(**depth_sil_rendervar)
        depth = depth_sil[0, :, :].unsqueeze(0)
        return {"render": im, "depth": depth}

    # -- small surface ---------------------------------------------------------------------------------
    @property
    def cur_frame_idx(self):
        return self.frame_idx

    def get_gaussian_xyz(self):
        return self.params['means3D']

    @property
    def gaussian_points(self):
        return self.get_gaussian_xyz()

    def pause(self):
        """ API to be compatible with Mono GS """
        return

    def resume(self):
        """ API to be compatible with Mono GS """
        return

    def color_refinement(self):
        """ API to be compatible with Mono GS """
        return

    def stop(self):
        """ API to be compatible with Mono GS """
        return
