"""The object-aware training step (fr_loss_mask, fr_bg_penalty_forward / _backward, fr_outside_mask, include/fisher_rast.h) on torch
tensors: the loss pixel mask of get_loss, the two background penalties of the object class as an autograd function, and the mask of
the Gaussians that project outside the object mask.  No host synchronisation on the way: a mask goes to the kernels as bytes and
comes back as bytes, counts and ranges stay on the device in a status block.

Inputs the kernels do not take (not float32, not contiguous, not on one HIP device, shapes that do not fit) raise
`ObjectLossUnsupported` before anything is launched, so a caller may take the torch route for that call; there is no torch fallback
in here."""
import ctypes

import torch

from fisher_rast import _lib
from fisher_rast._lib import FisherRastError

OUTLIER_RATIO = 10.0          # the reference's `10 * depth_error.median()`


class ObjectLossUnsupported(FisherRastError):
    """the inputs are outside what the kernels take: raised before anything is launched"""


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _check_f32(dev, **tensors):
    """every tensor contiguous float32 on the HIP device `dev` (None: that of the first), or ObjectLossUnsupported; returns the device"""
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor):
            raise ObjectLossUnsupported(f"object loss: {name} must be a tensor")
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ObjectLossUnsupported(f"object loss: {name} must be contiguous float32 (got {t.dtype}, contiguous={t.is_contiguous()})")
        if not t.is_cuda:
            raise ObjectLossUnsupported(f"object loss: {name} must live on a HIP device")
        if dev is not None and t.device != dev:
            raise ObjectLossUnsupported(f"object loss: {name} is on {t.device}, other inputs on {dev}")
        dev = t.device
    return dev


def mask_bytes(obj_mask, H, W, dev):
    """The object mask as contiguous bytes [H,W] on `dev` (bool is reinterpreted, not copied; uint8 is taken as it is; anything
    else is `!= 0`), from [H,W] or [H,W,1] on either device.  None stays None."""
    if obj_mask is None:
        return None
    m = obj_mask
    if m.dim() == 3 and m.shape[-1] == 1:
        m = m.squeeze(-1)
    if tuple(m.shape) != (H, W):
        raise ObjectLossUnsupported(f"object loss: an object mask of {tuple(obj_mask.shape)} does not fit an image of {H} x {W}")
    if m.dtype not in (torch.bool, torch.uint8):
        m = m != 0
    if m.device != dev:
        m = m.to(dev)
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def _image_shape(depth_sil):
    if depth_sil.dim() != 3 or depth_sil.shape[0] != 3 or depth_sil.numel() == 0:
        raise ObjectLossUnsupported(f"object loss: depth_sil must be [3,H,W] (got {tuple(depth_sil.shape)})")
    H, W = int(depth_sil.shape[1]), int(depth_sil.shape[2])
    if H * W > 1 << 30:
        raise ObjectLossUnsupported("object loss: H W at most 2^30")
    return H, W


def loss_mask_raw(depth_sil, gt_depth, sil_thres, reject_outliers, need_presence, obj_bytes=None, outlier_ratio=OUTLIER_RATIO):
    """One fr_loss_mask call on checked tensors: (mask bytes [H,W], status int32 [5]), both on the device."""
    H, W = int(depth_sil.shape[1]), int(depth_sil.shape[2])
    dev = depth_sil.device
    lib = _lib.load()
    mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
    status = torch.empty((_lib.FR_LOSS_MASK_STATUS_WORDS,), dtype=torch.int32, device=dev)
    nws = int(lib.fr_loss_mask_workspace_bytes(H, W)) if reject_outliers else 0
    ws = torch.empty((nws // 8,), dtype=torch.int64, device=dev) if nws else None
    cfg = _lib.LossMaskCfg(H, W, float(sil_thres), int(bool(reject_outliers)), float(outlier_ratio), int(bool(need_presence)))
    with torch.cuda.device(dev):
        _lib.check(lib.fr_loss_mask(ctypes.byref(cfg), depth_sil.data_ptr(), gt_depth.data_ptr(), None if obj_bytes is None else obj_bytes.data_ptr(),
                                    mask.data_ptr(), status.data_ptr(), None if ws is None else ws.data_ptr(), nws, _stream(dev)), "fr_loss_mask")
    return mask, status


def loss_pixel_mask(depth_sil, gt_depth, sil_thres, reject_outliers, need_presence, obj_mask=None):
    """The pixels that enter the tracking / mapping loss -- `_loss_pixel_mask` of models/SLAM/gaussian.py with the object mask of
    models/SLAM/gaussian_object.py:236-248 ANDed in where one is given -- in one launch, five with `reject_outliers` (the median is a
    radix select, not a sort).  Returns (rendered depth [1,H,W], a view of `depth_sil`; mask bool [1,H,W], the kernel's bytes viewed
    as bool)."""
    ds = depth_sil.detach() if isinstance(depth_sil, torch.Tensor) else depth_sil
    dev = _check_f32(None, depth_sil=ds, gt_depth=gt_depth)
    H, W = _image_shape(ds)
    if gt_depth.numel() != H * W:
        raise ObjectLossUnsupported(f"object loss: a depth of {tuple(gt_depth.shape)} does not fit a render of {H} x {W}")
    obj = mask_bytes(obj_mask, H, W, dev)
    mask, _ = loss_mask_raw(ds, gt_depth.detach(), sil_thres, reject_outliers, need_presence, obj)
    return depth_sil[0:1], mask.view(torch.bool).unsqueeze(0)


def penalty_forward_raw(im, depth_sil, obj_bytes, lambda_rgb, lambda_alpha):
    """One fr_bg_penalty_forward call on checked tensors: (out4, saved2)."""
    H, W = int(im.shape[1]), int(im.shape[2])
    dev = im.device
    lib = _lib.load()
    out4 = torch.empty((4,), dtype=torch.float32, device=dev)
    saved2 = torch.empty((2,), dtype=torch.float32, device=dev)
    nws = int(lib.fr_bg_penalty_workspace_bytes(H, W))
    ws = torch.empty((nws // 8,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_bg_penalty_forward(H, W, float(lambda_rgb), float(lambda_alpha), im.data_ptr(), depth_sil.data_ptr(), obj_bytes.data_ptr(),
                                             out4.data_ptr(), saved2.data_ptr(), ws.data_ptr(), nws, _stream(dev)), "fr_bg_penalty_forward")
    return out4, saved2


def penalty_backward_raw(im, depth_sil, obj_bytes, lambda_rgb, lambda_alpha, saved2, upstream):
    """One fr_bg_penalty_backward call: (dL_dim, dL_ddepth_sil); `upstream` is a device float32 tensor whose first element is read."""
    H, W = int(im.shape[1]), int(im.shape[2])
    dev = im.device
    g_im, g_ds = torch.empty_like(im), torch.empty_like(depth_sil)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_bg_penalty_backward(H, W, float(lambda_rgb), float(lambda_alpha), im.data_ptr(), depth_sil.data_ptr(),
                                                      obj_bytes.data_ptr(), saved2.data_ptr(), upstream.data_ptr(), g_im.data_ptr(), g_ds.data_ptr(),
                                                      _stream(dev)), "fr_bg_penalty_backward")
    return g_im, g_ds


class _BackgroundPenalty(torch.autograd.Function):
    """out4[0] of one forward call as a 0-dim tensor, with its gradient to the colour render and to the depth / silhouette render"""

    @staticmethod
    def forward(ctx, im, depth_sil, obj_bytes, lambda_rgb, lambda_alpha):
        x, ds = im.detach(), depth_sil.detach()
        out4, saved2 = penalty_forward_raw(x, ds, obj_bytes, lambda_rgb, lambda_alpha)
        ctx.save_for_backward(x, ds, obj_bytes, saved2)
        ctx.lambdas = (float(lambda_rgb), float(lambda_alpha))
        return out4[0]

    @staticmethod
    def backward(ctx, grad_out):
        x, ds, obj_bytes, saved2 = ctx.saved_tensors
        up = grad_out if (grad_out.dtype == torch.float32 and grad_out.is_contiguous()) else grad_out.float().contiguous()
        g_im, g_ds = penalty_backward_raw(x, ds, obj_bytes, ctx.lambdas[0], ctx.lambdas[1], saved2, up.reshape(1))
        return g_im, g_ds, None, None, None


def background_penalty(im, depth_sil, obj_mask, lambda_rgb=0.1, lambda_alpha=0.1):
    """lambda_rgb * mean |im| + lambda_alpha * mean clamp(silhouette, 0, 1), both over the pixels outside the object mask
    (models/SLAM/gaussian_object.py:263-275), as a 0-dim tensor that is differentiable w.r.t. `im` [3,H,W] and `depth_sil` [3,H,W]
    (its channel 1).  Two launches forward, one backward."""
    dev = _check_f32(None, im=im, depth_sil=depth_sil)
    H, W = _image_shape(depth_sil)
    if tuple(im.shape) != (3, H, W):
        raise ObjectLossUnsupported(f"object loss: im must be [3,{H},{W}] (got {tuple(im.shape)})")
    if obj_mask is None:
        raise ObjectLossUnsupported("object loss: the background penalty needs an object mask")
    return _BackgroundPenalty.apply(im, depth_sil, mask_bytes(obj_mask, H, W, dev), lambda_rgb, lambda_alpha)


def outside_mask(params, w2c, intrinsics, obj_mask):
    """Which Gaussians of `params` do not project into `obj_mask` under the pose `w2c` [4,4] and `intrinsics` [3,3]
    (models/SLAM/utils/slam_external.py:290-315).  Returns (outside bool [P], status int32 [6] on the device: in_count, out_count
    and the bits of the scale ranges, fr_outside_mask).  Two launches, no host read."""
    means, logs = params['means3D'].detach(), params['log_scales'].detach()
    dev = _check_f32(None, means3D=means, log_scales=logs)
    if means.dim() != 2 or means.shape[1] != 3 or logs.dim() != 2 or logs.shape[0] != means.shape[0] or int(logs.shape[1]) not in (1, 3):
        raise ObjectLossUnsupported(f"object loss: means3D [P,3] and log_scales [P,1] or [P,3] (got {tuple(means.shape)}, {tuple(logs.shape)})")
    if obj_mask is None or not (obj_mask.dim() == 2 or (obj_mask.dim() == 3 and obj_mask.shape[-1] == 1)) or obj_mask.numel() == 0:
        raise ObjectLossUnsupported("object loss: the outside mask needs an object mask [H,W] or [H,W,1]")
    H, W = int(obj_mask.shape[0]), int(obj_mask.shape[1])
    obj = mask_bytes(obj_mask, H, W, dev)
    cam = []
    for name, t, shape in (("w2c", w2c, (4, 4)), ("intrinsics", intrinsics, (3, 3))):
        t = torch.as_tensor(t).detach()
        if tuple(t.shape) != shape:
            raise ObjectLossUnsupported(f"object loss: {name} must be {list(shape)} (got {tuple(t.shape)})")
        cam.append(t.to(device=dev, dtype=torch.float32).contiguous())
    P = int(means.shape[0])
    lib = _lib.load()
    outside = torch.empty((P,), dtype=torch.uint8, device=dev)
    status = torch.empty((_lib.FR_OUTSIDE_STATUS_WORDS,), dtype=torch.int32, device=dev)
    nws = int(lib.fr_outside_mask_workspace_bytes(P))
    ws = torch.empty((nws // 8,), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_outside_mask(P, int(logs.shape[1]), means.data_ptr(), logs.data_ptr(), cam[0].data_ptr(), cam[1].data_ptr(), obj.data_ptr(),
                                       H, W, outside.data_ptr(), status.data_ptr(), ws.data_ptr(), nws, _stream(dev)), "fr_outside_mask")
    return outside.view(torch.bool), status
