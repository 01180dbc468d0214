"""The fused image loss (fr_image_loss_forward / fr_image_loss_backward, include/fisher_rast.h) as torch autograd functions:
w_l1 * L1 + w_ssim * (1 - SSIM) between a render and its target, two launches forward and one backward per term, with no host
synchronisation on the way (no `.item()`, no boolean indexing: a mask goes to the kernels as bytes).

`image_loss(...)` is what `models/SLAM/utils/slam_helpers.py` (calc_loss, calc_loss_mask, l1_loss_v1) and
`models/SLAM/utils/slam_external.py` (calc_ssim, calc_ssim_masked) are written on; `forward_raw` / `backward_raw` are the two ABI
calls on plain tensors, for tests and tools.  There is no torch fallback: without the library every call raises."""
import ctypes

import torch

from fisher_rast import _lib
from fisher_rast._lib import FR_LOSS_L1_MASKED_MEAN, FR_LOSS_L1_MEAN, FR_LOSS_L1_SUM   # noqa: F401

OUT_LOSS, OUT_L1, OUT_SSIM, OUT_COUNT = 0, 1, 2, 3


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _f32(t):
    return t if (t.dtype == torch.float32 and t.is_contiguous()) else t.float().contiguous()


def _mask_bytes(mask, C, H, W):
    """The mask as contiguous bytes [C,H,W] or [1,H,W] (bool is reinterpreted, not copied); returns (tensor, mask_channels)."""
    if mask is None:
        return None, 0
    m = mask if mask.dtype in (torch.bool, torch.uint8) else (mask != 0)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    m = m.reshape(-1, H, W).contiguous()
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.shape[0] not in (1, C):
        raise ValueError(f"image loss: a mask of {tuple(mask.shape)} does not fit an image of [{C},{H},{W}]")
    return m, (1 if m.shape[0] == 1 and C != 1 else C)


def _cfg(C, H, W, w_l1, w_ssim, denom, mask_channels, weights_map):
    return _lib.ImageLossCfg(C, H, W, float(w_l1), float(w_ssim), int(denom), int(mask_channels), int(bool(weights_map)))


def saved_floats(C, H, W, w_ssim):
    return (3 * C * H * W if float(w_ssim) != 0.0 else 0) + 4


def forward_raw(img, gt, mask=None, w_l1=1.0, w_ssim=0.0, denom=FR_LOSS_L1_MEAN, weights_map=False, want_map=False,
                want_channels=False):
    """One fr_image_loss_forward call on [C,H,W] float32 device tensors.  Returns (out4, channel_ssim or None, ssim_map or None,
    saved, cfg, mask bytes) -- the last three are what `backward_raw` takes."""
    C, H, W = (int(s) for s in img.shape)
    dev = img.device
    m, mc = _mask_bytes(mask, C, H, W)
    cfg = _cfg(C, H, W, w_l1, w_ssim, denom, mc, weights_map)
    lib = _lib.load()
    out4 = torch.empty((4,), dtype=torch.float32, device=dev)
    chan = torch.empty((C,), dtype=torch.float32, device=dev) if want_channels else None
    smap = torch.empty((C, H, W), dtype=torch.float32, device=dev) if want_map else None
    saved = torch.empty((saved_floats(C, H, W, w_ssim),), dtype=torch.float32, device=dev)
    nws = int(lib.fr_image_loss_workspace_bytes(C, H, W))
    ws = torch.empty((nws // 8,), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_image_loss_forward(ctypes.byref(cfg), img.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(),
                                             out4.data_ptr(), None if chan is None else chan.data_ptr(),
                                             None if smap is None else smap.data_ptr(), saved.data_ptr(), ws.data_ptr(), nws, _stream(dev)),
                   "fr_image_loss_forward")
    return out4, chan, smap, saved, cfg, m


def backward_raw(img, gt, m, saved, cfg, upstream):
    """One fr_image_loss_backward call; `upstream` is a device float32 tensor whose first element is read by the kernel."""
    dev = img.device
    grad = torch.empty_like(img)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_image_loss_backward(ctypes.byref(cfg), img.data_ptr(), gt.data_ptr(), None if m is None else m.data_ptr(),
                                                      saved.data_ptr(), upstream.data_ptr(), grad.data_ptr(), _stream(dev)),
                   "fr_image_loss_backward")
    return grad


class _ImageLoss(torch.autograd.Function):
    """out4[which] of one forward call as a 0-dim tensor (plus the per-channel SSIM means and the map when asked), with the
    gradient of `out4[OUT_LOSS]` to the render.  Callers that return the SSIM mean itself pass w_l1 = 0, w_ssim = -1: the loss is
    then ssim - 1, whose gradient is the SSIM mean's."""

    @staticmethod
    def forward(ctx, img, gt, mask, w_l1, w_ssim, denom, weights_map, which, want_map, want_channels):
        if ctx.needs_input_grad[1]:
            raise NotImplementedError("image loss: a gradient to the target image is not built (detach it)")
        shape = img.shape
        H, W = int(shape[-2]), int(shape[-1])
        x = _f32(img.detach()).reshape(-1, H, W)            # a batch folds into the channels
        y = _f32(gt.detach()).reshape(-1, H, W)
        if x.shape != y.shape:
            raise ValueError(f"image loss: render {tuple(img.shape)} and target {tuple(gt.shape)} differ")
        out4, chan, smap, saved, cfg, m = forward_raw(x, y, mask, w_l1, w_ssim, denom, weights_map, want_map, want_channels)
        ctx.save_for_backward(x, y, saved, m if m is not None else x.new_empty(0))
        ctx.cfg, ctx.shape, ctx.dtype = cfg, shape, img.dtype
        if smap is not None:
            smap = smap.reshape(shape)
        ctx.mark_non_differentiable(*(t for t in (chan, smap) if t is not None))
        return out4[which], chan, smap

    @staticmethod
    def backward(ctx, grad_out, _gc, _gm):
        x, y, saved, m = ctx.saved_tensors
        up = _f32(grad_out).reshape(1)
        grad = backward_raw(x, y, m if m.numel() else None, saved, ctx.cfg, up).reshape(ctx.shape)
        if grad.dtype != ctx.dtype:
            grad = grad.to(ctx.dtype)
        return (grad,) + (None,) * 9


def image_loss(img, gt, mask=None, w_l1=1.0, w_ssim=0.0, denom=FR_LOSS_L1_MEAN, weights_map=False, which=OUT_LOSS,
               want_map=False, want_channels=False):
    """(value, channel SSIM means or None, SSIM map or None); `value` is differentiable w.r.t. `img`."""
    if not img.is_cuda:
        raise _lib.FisherRastError("image loss: the tensors must be on the GPU (there is no CPU fallback for this path)")
    return _ImageLoss.apply(img, gt, mask, w_l1, w_ssim, denom, weights_map, which, want_map, want_channels)
