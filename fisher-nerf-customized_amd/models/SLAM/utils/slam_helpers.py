"""Render-variable builders on the hot path (models/SLAM/utils/slam_helpers.py:178-188, 235-252, 268-279), their fused form on the
render-variable kernels (fisher_rast/rendervar.py: frame_render_vars, transform_to_frame) and the loss terms of the training step
(slam_helpers.py:5-6, 23-77) on the fused image-loss kernels (fisher_rast/image_loss.py)."""
import torch
import torch.nn.functional as F

from fisher_rast import image_loss as _il
from fisher_rast import rendervar as _rv


def _scales3(params):
    ls = params['log_scales']
    return ls if ls.shape[-1] == 3 else torch.tile(ls, (1, 3))


def transformed_params2rendervar(params, transformed_pts):
    return {
        'means3D': transformed_pts,
        'colors_precomp': params['rgb_colors'],
        'rotations': F.normalize(params['unnorm_rotations']),
        'opacities': torch.sigmoid(params['logit_opacities']),
        'scales': torch.exp(_scales3(params)),
        'means2D': torch.zeros_like(params['means3D'], requires_grad=True) + 0,
    }


def get_depth_and_silhouette(pts_3D, w2c):
    """Per-Gaussian "colour" (z, 1, z^2) used for the depth + silhouette render."""
    pts4 = torch.cat((pts_3D, torch.ones_like(pts_3D[:, :1])), dim=-1)
    z = (w2c @ pts4.transpose(0, 1)).transpose(0, 1)[:, 2:3]
    return torch.cat((z, torch.ones_like(z), torch.square(z)), dim=1).float()


def transformed_params2depthplussilhouette(params, w2c, transformed_pts):
    return {
        'means3D': transformed_pts,
        'colors_precomp': get_depth_and_silhouette(transformed_pts, w2c),
        'rotations': F.normalize(params['unnorm_rotations']),
        'opacities': torch.sigmoid(params['logit_opacities']),
        'scales': torch.exp(_scales3(params)),
        'means2D': torch.zeros_like(params['means3D'], requires_grad=True) + 0,
    }


def frame_render_vars(params, time_idx, w2c, gaussians_grad, camera_grad):
    """transform_to_frame (slam_helpers.py:282-317), transformed_params2rendervar and get_depth_and_silhouette in one launch
    (`FrameRenderVars`): (rendervar, feats), `rendervar` with the keys of transformed_params2rendervar ('means2D' the torch leaf it
    is there) and `feats` the (z, 1, z^2) features of the depth / silhouette render under the first frame's `w2c`.  Raises
    `RenderVarUnsupported` on inputs the kernels do not take (not float32, not contiguous, not on one HIP device, log_scales not 1 or 3
    wide)."""
    pts, feats, rotations, opacities, scales = _rv.FrameRenderVars.apply(
        params['means3D'], params['unnorm_rotations'], params['logit_opacities'], params['log_scales'],
        params['cam_unnorm_rots'], params['cam_trans'], time_idx, w2c, gaussians_grad, camera_grad)
    rendervar = {
        'means3D': pts,
        'colors_precomp': params['rgb_colors'],
        'rotations': rotations,
        'opacities': opacities,
        'scales': scales,
        'means2D': torch.zeros_like(params['means3D'], requires_grad=True) + 0,
    }
    return rendervar, feats


def transform_to_frame(params, time_idx, gaussians_grad, camera_grad):
    """Drop-in for the reference's transform_to_frame (slam_helpers.py:282-317) on the same kernel, with only the points asked for."""
    return _rv.FrameRenderVars.apply(params['means3D'], None, None, None, params['cam_unnorm_rots'], params['cam_trans'], time_idx, None,
                                     gaussians_grad, camera_grad)[0]


def render_rgb_depth_sil(params, cam, w2c, transformed_pts, renderer_cls=None, rendervar=None, feats=None):
    """The two renders of the reference's get_loss (models/SLAM/gaussian.py:199-211) -- RGB, then (depth, silhouette, depth^2)
    on the same Gaussians -- as one call on one projection / binning / sort (`GaussianRasterizer.forward_pair`).
    Returns (im [3,H,W], radius [P], depth_sil [3,H,W], rendervar); `rendervar['means2D']` keeps the colour render's
    screen-space gradient, the statistic the densifier accumulates (gaussian.py:207).  `rendervar` / `feats` prebuilt
    (`frame_render_vars`) are taken as they are instead of being built here."""
    if renderer_cls is None:
        from diff_gaussian_rasterization import GaussianRasterizer as renderer_cls
    if rendervar is None:
        rendervar = transformed_params2rendervar(params, transformed_pts)
    rendervar['means2D'].retain_grad()
    if feats is None:
        feats = get_depth_and_silhouette(transformed_pts, w2c)
    im, radius, _, depth_sil = renderer_cls(raster_settings=cam).forward_pair(
        rendervar['means3D'], rendervar['means2D'], rendervar['opacities'], rendervar['colors_precomp'], feats,
        scales=rendervar['scales'], rotations=rendervar['rotations'])
    return im, radius, depth_sil, rendervar


def l1_loss_v1(x, y):
    """slam_helpers.py:5-6: mean |x - y|, differentiable w.r.t. x ([C,H,W] or [B,C,H,W])."""
    return _il.image_loss(x, y, None, 1.0, 0.0, _il.FR_LOSS_L1_MEAN)[0]


def _loss_terms(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking, mask_colour):
    losses = {}
    if use_l1:
        # depth: the masked sum in tracking, the masked mean in mapping
        losses['depth'] = _il.image_loss(depth, curr_data['depth'], mask.detach(), 1.0, 0.0,
                                         _il.FR_LOSS_L1_SUM if tracking else _il.FR_LOSS_L1_MASKED_MEAN)[0]
    if tracking and (use_sil_for_loss or ignore_outlier_depth_loss):
        losses['im'] = _il.image_loss(im, curr_data['im'], color_mask, 1.0, 0.0, _il.FR_LOSS_L1_SUM)[0]
    elif tracking:
        losses['im'] = _il.image_loss(im, curr_data['im'], None, 1.0, 0.0, _il.FR_LOSS_L1_SUM)[0]
    elif mask_colour:
        # the masked mean of |.| and the SSIM of the two images times the mask
        losses['im'] = _il.image_loss(im, curr_data['im'], color_mask, 0.8, 0.2, _il.FR_LOSS_L1_MASKED_MEAN)[0]
    else:
        losses['im'] = _il.image_loss(im, curr_data['im'], None, 0.8, 0.2, _il.FR_LOSS_L1_MEAN)[0]
    return losses


def calc_loss(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking):
    """slam_helpers.py:23-44: {'depth': .., 'im': ..}, each entry one forward launch pair and one backward launch."""
    return _loss_terms(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking, False)


def calc_loss_mask(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking):
    """slam_helpers.py:46-77: calc_loss with the mapping colour term taken over `color_mask` only."""
    return _loss_terms(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking, True)
