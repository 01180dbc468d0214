"""Torch-tensor front end of the C ABI: device memory, streams and nothing else.

Four groups of entry points:
  * `rasterize_forward` / `rasterize_backward` / `mark_visible` -- the argument lists of the reference's
    pybind module `_C` (thirdparty/diff-gaussian-rasterization-modified/ext.cpp:14-18,
    rasterize_points.h:18-66); `diff_gaussian_rasterization/_C.py` re-exports them under the reference names.
  * `FisherScorer` -- the batched multi-view scorer behind GaussianSLAM.compute_Hessian / compute_H_train /
    pose_eval (models/SLAM/gaussian.py:1338-1375, 1503-1570); its `render_views` renders a batch of poses in one call
    (RGB, depth / silhouette, median depth, final transmittance: fr_render_views); its `visible` / `popgs_block_prior` /
    `popgs_block_scores` are the POp-GS block stage (fr_raster_cfg.ext: fr_fisher_views renders nothing).
  * `knn_dist2` -- simple_knn._C.distCUDA2.
  * `popgs_diag_criterion` -- the POp-GS T-opt / D-opt score of a batch of views from their probe rows, and the priors of the
    path evaluation updated in the same pass (tester_gaussians_navigation.py:2147-2178).
  * `frame_ingest_select` / `frame_ingest_emit` -- which cells of an RGB-D frame become new Gaussians, and their parameter rows
    (models/SLAM/gaussian.py:320-414, 75-143, 299-318).
  * `keyframe_valid_pixels` / `keyframe_overlap` -- the pixels of a frame with a measured depth, and how many of the points drawn from
    them each keyframe sees (models/SLAM/utils/keyframe_selection.py:10-37, 40-134).
  * `view_metrics` / `view_metrics_summary` -- PSNR, SSIM and depth error of a batch of rendered views against their ground truth
    (tester_gaussians_navigation.py:1450-1491, models/SLAM/utils/eval_helpers.py:230-257).
"""
import ctypes
from typing import Optional

import torch

from . import _lib
from ._lib import FisherRastError, RasterCfg, Gaussians, FisherCfg, FrameIngestCfg, KeyframeCfg


def _need_gpu(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise FisherRastError(f"{name} must live on a HIP device; fisher_rast has no CPU path")


def _prep(t: Optional[torch.Tensor], device) -> Optional[torch.Tensor]:
    """contiguous fp32 on `device`; the reference's empty tensors (any device) become None -> null pointer."""
    if t is None or t.numel() == 0:
        return None
    if t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _raster_cfg(P, H, W, tanfovx, tanfovy, scale_modifier, degree, M, prefiltered, bg, view, proj, campos):
    c = RasterCfg()
    c.P, c.image_height, c.image_width = int(P), int(H), int(W)
    c.tanfovx, c.tanfovy, c.scale_modifier = float(tanfovx), float(tanfovy), float(scale_modifier)
    c.sh_degree, c.sh_coeffs, c.prefiltered = int(degree), int(M), int(bool(prefiltered))
    c.bg, c.viewmatrix, c.projmatrix, c.campos = _ptr(bg), _ptr(view), _ptr(proj), _ptr(campos)
    return c


def _gaussians(means3D, colors, sh, opacity, scales, rotations, cov3D):
    g = Gaussians()
    g.means3D, g.colors_precomp, g.shs = _ptr(means3D), _ptr(colors), _ptr(sh)
    g.opacities, g.scales, g.rotations, g.cov3D_precomp = _ptr(opacity), _ptr(scales), _ptr(rotations), _ptr(cov3D)
    return g


def workspace_bytes(P, W, H, max_rendered):
    out = (ctypes.c_size_t * 3)()
    _lib.check(_lib.load().fr_workspace_bytes(P, W, H, max_rendered, out), "fr_workspace_bytes")
    return int(out[0]), int(out[1]), int(out[2])


def workspace_layout(P, W, H, max_rendered):
    names = ("splat", "cov3D", "rgb", "clamped",
             "tile_count", "tile_offset", "tile_fill", "final_T", "n_contrib", "status", "keys")
    out = (ctypes.c_size_t * 11)()
    _lib.check(_lib.load().fr_workspace_layout(P, W, H, max_rendered, out), "fr_workspace_layout")
    return {n: int(out[i]) for i, n in enumerate(names)}


# high-water mark of tile instances per device, so that the binning buffer is normally large enough first time
# (host integers only, no device memory: shared by every stream and thread -- a stale or lost update costs one re-run of a forward)
_capacity_hint = {}


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:198-217)."""
    _need_gpu(means3D, "means3D")
    dev = means3D.device
    P = means3D.shape[0]
    present = torch.zeros((P,), dtype=torch.bool, device=dev)
    if P != 0:
        m, v, pr = _prep(means3D, dev), _prep(viewmatrix, dev), _prep(projmatrix, dev)
        with torch.cuda.device(dev):
            _lib.check(_lib.load().fr_mark_visible(P, _ptr(m), _ptr(v), _ptr(pr), ctypes.c_void_p(present.data_ptr()),
                                                   _stream(dev)), "fr_mark_visible")
    return present


def rasterize_forward(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                      viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                      prefiltered, features=None):
    """RasterizeGaussiansCUDA (rasterize_points.cu:35-115): returns
    (num_rendered, color[3,H,W], radii[P] int32, geomBuffer, binningBuffer, imgBuffer, depth[1,H,W])."""
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _need_gpu(means3D, "means3D")
    dev = means3D.device
    lib = _lib.load()
    P, H, W = int(means3D.shape[0]), int(image_height), int(image_width)
    means3D = _prep(means3D, dev)
    colors, sh_t = _prep(colors, dev), _prep(sh, dev)
    opacity, scales, rotations, cov3D_precomp = (_prep(opacity, dev), _prep(scales, dev), _prep(rotations, dev),
                                                 _prep(cov3D_precomp, dev))
    bg, view, proj, cpos = _prep(background, dev), _prep(viewmatrix, dev), _prep(projmatrix, dev), _prep(campos, dev)
    M = int(sh.shape[1]) if (sh is not None and sh.numel() != 0) else 0

    out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    out_depth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
    # `features` (not in the reference's argument list): a second [P,3] array composited in the same pass (fr_forward_pair);
    # its image is appended to the returned tuple
    feats = _prep(features, dev) if features is not None else None
    out_feat = torch.empty((3, H, W), dtype=torch.float32, device=dev) if features is not None else None
    radii = torch.zeros((P,), dtype=torch.int32, device=dev)
    status = torch.zeros((4,), dtype=torch.int32, device=dev)
    cfg = _raster_cfg(P, H, W, tan_fovx, tan_fovy, scale_modifier, degree, M, prefiltered, bg, view, proj, cpos)
    g = _gaussians(means3D, colors, sh_t, opacity, scales, rotations, cov3D_precomp)

    key = (dev.index, P, H, W)
    capacity = max(_capacity_hint.get(key, 0), 2 * P, 1 << 16)
    with torch.cuda.device(dev):
        while True:
            gb, bb, ib = workspace_bytes(P, W, H, capacity)
            geom = torch.empty((gb,), dtype=torch.uint8, device=dev)
            binning = torch.empty((bb,), dtype=torch.uint8, device=dev)
            img = torch.empty((ib,), dtype=torch.uint8, device=dev)
            if features is not None:
                _lib.check(lib.fr_forward_pair(ctypes.byref(cfg), ctypes.byref(g), _ptr(feats), geom.data_ptr(), binning.data_ptr(),
                                               capacity, img.data_ptr(), _ptr(out_color), _ptr(out_feat), _ptr(out_depth),
                                               radii.data_ptr(), status.data_ptr(), _stream(dev)), "fr_forward_pair")
            else:
                _lib.check(lib.fr_forward(ctypes.byref(cfg), ctypes.byref(g), geom.data_ptr(), binning.data_ptr(), capacity,
                                          img.data_ptr(), _ptr(out_color), _ptr(out_depth), radii.data_ptr(),
                                          status.data_ptr(), _stream(dev)), "fr_forward")
            # same host synchronisation as the reference (rasterizer_impl.cu:282: cudaMemcpy of num_rendered)
            st = status.cpu()
            num_rendered = int(st[0])
            if int(st[3]):
                # auxiliary.h:156-160 prints this and traps the device; here the call fails and the device stays usable
                raise RuntimeError("Point is filtered although prefiltered is set. This shouldn't happen!")
            if int(st[1]) == 0:
                break
            capacity = int(num_rendered * 1.25) + 1024
    _capacity_hint[key] = max(_capacity_hint.get(key, 0), int(num_rendered * 1.25) + 1024)
    if features is not None:
        return num_rendered, out_color, radii, geom, binning, img, out_depth, out_feat
    return num_rendered, out_color, radii, geom, binning, img, out_depth


_bwd_scratch = {}


def _backward_scratch(dev, nbytes):
    """The scratch of the chunked power-2 backward, kept per (device, stream) and only ever grown: 56 MB for a 256 x 256 view of the
    benchmark room, 0.5 GB for 2M Gaussians at 512 x 512 -- a fresh `torch.empty` of that size per call sent the caching allocator
    through free / malloc cycles when image sizes alternate (1.8 ms per call instead of 0.45).  `release_backward_scratch()` drops it."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(dev).cuda_stream))
    t = _bwd_scratch.get(key)
    if t is None or t.numel() < nbytes:
        _bwd_scratch[key] = None
        t = torch.empty((nbytes + (nbytes >> 2),), dtype=torch.uint8, device=dev)
        _bwd_scratch[key] = t
    return t


def release_backward_scratch():
    _bwd_scratch.clear()


def rasterize_backward(background, means3D, radii, colors, scales, rotations, scale_modifier, cov3D_precomp,
                       viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, geomBuffer,
                       R, binningBuffer, imageBuffer, power, opacities=None, segmented=True):
    """RasterizeGaussiansBackwardCUDA (rasterize_points.cu:117-196): returns
    (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations).
    `segmented=False` withholds the scratch buffer of the power-2 backward (tests: the single-pass walk)."""
    _need_gpu(means3D, "means3D")
    dev = means3D.device
    lib = _lib.load()
    P = int(means3D.shape[0])
    H, W = int(dL_dout_color.shape[1]), int(dL_dout_color.shape[2])
    M = int(sh.shape[1]) if (sh is not None and sh.numel() != 0) else 0
    means3D = _prep(means3D, dev)
    colors, sh_t = _prep(colors, dev), _prep(sh, dev)
    scales, rotations, cov3D_precomp = _prep(scales, dev), _prep(rotations, dev), _prep(cov3D_precomp, dev)
    bg, view, proj, cpos = _prep(background, dev), _prep(viewmatrix, dev), _prep(projmatrix, dev), _prep(campos, dev)
    dL = _prep(dL_dout_color, dev)

    def new(*shape):
        return torch.empty(shape, dtype=torch.float32, device=dev)
    dL_dmeans3D, dL_dmeans2D, dL_dcolors = new(P, 3), new(P, 3), new(P, 3)
    dL_dconic, dL_dopacity, dL_dcov3D = new(P, 2, 2), new(P, 1), new(P, 6)
    dL_dsh, dL_dscales, dL_drotations = torch.zeros((P, M, 3), dtype=torch.float32, device=dev), new(P, 3), new(P, 4)
    if P != 0:
        # the kernels read opacity from the splat records of the geometry buffer
        opac = _prep(opacities, dev) if opacities is not None else None
        cfg = _raster_cfg(P, H, W, tan_fovx, tan_fovy, scale_modifier, degree, M, False, bg, view, proj, cpos)
        g = _gaussians(means3D, colors, sh_t, opac, scales, rotations, cov3D_precomp)
        # scratch for the chunked backward (fisher_rast.h, fr_backward_ws; power 1 and 2)
        nscr = int(lib.fr_backward_scratch_bytes(P, W, H, int(power), int(R))) if segmented else 0
        scratch = _backward_scratch(dev, nscr) if nscr else None
        with torch.cuda.device(dev):
            _lib.check(lib.fr_backward_ws(ctypes.byref(cfg), ctypes.byref(g), radii.data_ptr(), geomBuffer.data_ptr(),
                                          binningBuffer.data_ptr(), imageBuffer.data_ptr(), _ptr(dL), int(power),
                                          _ptr(dL_dmeans2D), _ptr(dL_dcolors), _ptr(dL_dopacity), _ptr(dL_dmeans3D),
                                          _ptr(dL_dcov3D), _ptr(dL_dsh) if M > 0 else None, _ptr(dL_dscales),
                                          _ptr(dL_drotations), _ptr(dL_dconic), int(R), scratch.data_ptr() if nscr else None,
                                          scratch.numel() if nscr else 0,
                                          _stream(dev)), "fr_backward")
    else:
        for t in (dL_dmeans3D, dL_dmeans2D, dL_dcolors, dL_dconic, dL_dopacity, dL_dcov3D, dL_dscales, dL_drotations):
            t.zero_()
    return dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, dL_drotations


def rasterize_forward_features(features, raster_cfg_args, geomBuffer, binningBuffer, imageBuffer):
    """A second [P,3] feature array composited over the geometry the last `rasterize_forward` binned
    (fr_forward_features): returns the [3,H,W] image.  raster_cfg_args = (P, H, W, tanfovx, tanfovy, scale_modifier, bg, view, proj, campos)."""
    P, H, W, tfx, tfy, mod, bg, view, proj, cpos = raster_cfg_args
    dev = geomBuffer.device if P else bg.device
    out = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    feats = _prep(features, dev)
    bg, view, proj, cpos = _prep(bg, dev), _prep(view, dev), _prep(proj, dev), _prep(cpos, dev)
    cfg = _raster_cfg(P, H, W, tfx, tfy, mod, 0, 0, False, bg, view, proj, cpos)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_forward_features(ctypes.byref(cfg), _ptr(feats), geomBuffer.data_ptr() if P else None,
                                                   binningBuffer.data_ptr() if P else None, imageBuffer.data_ptr() if P else None,
                                                   _ptr(out), _stream(dev)), "fr_forward_features")
    return out


def rasterize_backward_pair(background, means3D, radii, colors, features, scales, rotations, scale_modifier, cov3D_precomp,
                            viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color, dL_dout_features, campos,
                            geomBuffer, binningBuffer, imageBuffer, num_rendered=0, segmented=True):
    """Backward of (colour image, feature image) on shared geometry, grad_power 1 (fr_backward_pair): returns
    (dL_dmeans2D [colour image only], dL_dmeans2D_features, dL_dcolors, dL_dfeatures, dL_dopacity, dL_dmeans3D, dL_dcov3D,
     dL_dscales, dL_drotations)."""
    _need_gpu(means3D, "means3D")
    dev = means3D.device
    P = int(means3D.shape[0])
    H, W = int(dL_dout_color.shape[1]), int(dL_dout_color.shape[2])
    means3D, colors, feats = _prep(means3D, dev), _prep(colors, dev), _prep(features, dev)
    scales, rotations, cov3D_precomp = _prep(scales, dev), _prep(rotations, dev), _prep(cov3D_precomp, dev)
    bg, view, proj, cpos = _prep(background, dev), _prep(viewmatrix, dev), _prep(projmatrix, dev), _prep(campos, dev)
    dL, dLf = _prep(dL_dout_color, dev), _prep(dL_dout_features, dev)

    def new(*shape):
        return torch.zeros(shape, dtype=torch.float32, device=dev)
    m2, m2f, dc, df = new(P, 3), new(P, 3), new(P, 3), new(P, 3)
    dop, dm3, dcov, dsc, drot, dcon = new(P, 1), new(P, 3), new(P, 6), new(P, 3), new(P, 4), new(P, 2, 2)
    if P != 0:
        cfg = _raster_cfg(P, H, W, tan_fovx, tan_fovy, scale_modifier, 0, 0, False, bg, view, proj, cpos)
        g = _gaussians(means3D, colors, None, None, scales, rotations, cov3D_precomp)
        lib = _lib.load()
        # with the forward's num_rendered: scratch for the chunked form (fisher_rast.h, fr_backward_pair_ws)
        nscr = int(lib.fr_backward_pair_scratch_bytes(P, W, H, int(num_rendered))) if (segmented and num_rendered) else 0
        scratch = _backward_scratch(dev, nscr) if nscr else None
        with torch.cuda.device(dev):
            _lib.check(lib.fr_backward_pair_ws(ctypes.byref(cfg), ctypes.byref(g), radii.data_ptr(), geomBuffer.data_ptr(),
                                               binningBuffer.data_ptr(), imageBuffer.data_ptr(), _ptr(dL), _ptr(feats), _ptr(dLf),
                                               _ptr(m2), _ptr(m2f), _ptr(dc), _ptr(df), _ptr(dop), _ptr(dm3), _ptr(dcov),
                                               _ptr(dsc), _ptr(drot), _ptr(dcon), int(num_rendered), scratch.data_ptr() if nscr else None,
                                               scratch.numel() if nscr else 0, _stream(dev)), "fr_backward_pair")
    return m2, m2f, dc, df, dop, dm3, dcov, dsc, drot


class FisherScorer:
    """Batched Fisher-information scorer for one Gaussian map and one camera.

    Holds the activated render variables (what gaussian.py:1529-1543 builds per call) and a reusable
    workspace.  `run()` scores / accumulates any number of views with no host synchronisation; the caller
    synchronises when it reads the results.  Overflow of the tile-instance buffer is detected from the
    device status word when results are fetched (`fetch`), and the batch is re-run with a larger buffer.

    One scorer, one stream at a time: every call runs on the torch stream that is current when it is made, and the workspaces
    (`_ws`, one per kind of launch) and the packed static records in them are shared by the calls that follow each other -- they
    are NOT keyed by stream.  Calls made on different streams must be ordered by the caller (an event, `wait_stream`) exactly as
    two writers of one tensor would be; callers that want to score on two streams side by side build a scorer per stream.
    """

    WORKSPACE_BUDGET = 32 << 30  # bytes of workspace (of the MI355X's 288 GB) before views are processed in chunks: ~580 views at 500k Gaussians
    MAX_KEY_BYTES_PER_VIEW = 512 << 20  # fixed key segments beyond this per view: packed lists instead (tile_capacity = 0)

    def __init__(self, raster_settings, means3D, rgb_colors, rotations, opacities, scales, columns: int = 4,
                 dL_dpix: float = 1e-3, tile_capacity: int = -1, spatial_order: bool = False):
        _need_gpu(means3D, "means3D")
        if columns not in (4, 11):
            raise ValueError("columns must be 4 or 11")
        self.lib = _lib.load()
        self.dev = means3D.device
        self.rs = raster_settings
        self.columns = columns
        self.dL = float(dL_dpix)
        d = self.dev
        self.means3D, self.colors = _prep(means3D.detach(), d), _prep(rgb_colors.detach(), d)
        self.rotations, self.opacities = _prep(rotations.detach(), d), _prep(opacities.detach().reshape(-1), d)
        scales = scales.detach()
        if scales.dim() == 2 and scales.shape[-1] == 1:  # isotropic (gaussian.py:1532-1533)
            scales = torch.tile(scales, (1, 3))
        self.scales = _prep(scales, d)
        self.P = int(self.means3D.shape[0])
        self.H, self.W = int(raster_settings.image_height), int(raster_settings.image_width)
        self.bg = _prep(raster_settings.bg, d)
        self.view = _prep(raster_settings.viewmatrix, d)
        self.proj = _prep(raster_settings.projmatrix, d)
        self.campos = _prep(raster_settings.campos, d)
        # The camera of the scorer's callers has the identity as its view matrix (every candidate pose arrives through w2c): the
        # library then leaves the view products out of the projection front end (fr_fisher_cfg.view_is_identity).  One exact
        # comparison here, none per call; the library checks the matrix again and a wrong hint raises in `run`.
        self.view_is_identity = (self.view is not None and self.view.numel() == 16
                                 and bool(torch.equal(self.view.reshape(4, 4).cpu(), torch.eye(4, dtype=self.view.dtype))))
        self._ws = {}
        self._static_key, self._static_hinv = None, None
        self.per_view_capacity = int(max(0.75 * self.P, 1 << 16))
        # Fixed key segments (fr_fisher_cfg.tile_capacity): every (view, tile) owns `tile_capacity` key slots, the projection
        # kernel places the keys itself and the scan / scatter kernels drop out of the launch sequence.  16384 keys (the largest
        # list the in-LDS sort tiers take) x 8 B = 128 KiB per tile -- 32 MiB per 256 x 256 view of the 288 GB; a longer list
        # raises the overflow flag and `run` grows the segments, or goes back to packed lists where they would not fit.
        self.tiles = ((self.W + 15) // 16) * ((self.H + 15) // 16)
        # (default: 32768 keys -- the library then partitions every list of up to 16320 keys behind itself, k_sort_split + k_sort_parts, and the
        # 1024-thread bitonic tier and its side stream only see longer lists -- or 16384 where that would pass the cap per view)
        if tile_capacity < 0:
            tile_capacity = 32768 if self.tiles * 32768 * 8 <= self.MAX_KEY_BYTES_PER_VIEW else 16384
        self.tile_capacity = int(tile_capacity)            # 0: packed key lists
        if self.tiles * self.tile_capacity * 8 > self.MAX_KEY_BYTES_PER_VIEW:
            self.tile_capacity = 0
        self.cfg = _raster_cfg(self.P, self.H, self.W, raster_settings.tanfovx, raster_settings.tanfovy,
                               raster_settings.scale_modifier, raster_settings.sh_degree, 0,
                               raster_settings.prefiltered, self.bg, self.view, self.proj, self.campos)
        self.g = _gaussians(self.means3D, self.colors, None, self.opacities, self.scales, self.rotations, None)
        # spatial_order=True: the Gaussians along a Z-curve (fr_fisher_cfg.order), computed once per map; the library lays them out and
        # processes them in that order -- a projection workgroup's 256 Gaussians are then neighbours in space (whole groups fall outside a
        # view and are skipped, a workgroup's keys land in a handful of tiles, a tile's records sit side by side).  Inputs and outputs
        # keep the caller's indexing.  OFF by default: measured on MI355X (500k Gaussians x 64 views, profiles/r04_d_spatial_order.txt) the
        # tile kernel gains 3.7 % and the projection kernel 2.8 %, the gathering k_pack_static loses as much (51 against 22 us) -- and two
        # DISTINCT splats of bit-equal depth in one tile (about one pair per view) then composite in Z-curve order, not in the reference's
        # index order (scores move by ~1e-5; exact duplicates keep their order).
        # The order follows the means: `launch` / `pose_launch` take it again when the means' (address, version) has moved on.
        self.spatial_order = bool(spatial_order) and self.P > 0
        self.order, self._order_src = None, None
        self._sync_order()

    def _map_key(self):
        """(address, version) of every tensor the static records are built from: an in-place write through a tensor op bumps the
        version; a write that bypasses autograd's version counter (`.data`, collectives, DLPack, raw pointers) must be followed by
        `map_changed()`."""
        return tuple((t.data_ptr(), t._version) for t in (self.means3D, self.colors, self.rotations, self.opacities, self.scales, self.order)
                     if t is not None)

    def _sync_order(self, force=False):
        if not self.spatial_order:
            return
        src = (self.means3D.data_ptr(), self.means3D._version)
        if force or self.order is None or src != self._order_src:
            self.order, self._order_src = spatial_order_of(self.means3D), src

    def map_changed(self):
        """Tell the scorer that the tensors it holds were written behind autograd's version counter (`.data`, a collective, DLPack,
        a raw pointer): the next call packs its static records again, and the spatial order is taken again."""
        self._static_key, self._static_hinv = None, None
        self._sync_order(force=True)

    # -- helpers -------------------------------------------------------------------------------------
    def max_views_per_launch(self):
        """Views per fr_fisher_views call that keep the workspace within WORKSPACE_BUDGET (the per-view share is what the
        library itself reports: records, visible lists, keys, per-tile arrays)."""
        one = int(self.lib.fr_fisher_workspace_bytes(self.P, self.W, self.H, 1, self._keys_per_view(), self.columns))
        eight = int(self.lib.fr_fisher_workspace_bytes(self.P, self.W, self.H, 8, 8 * self._keys_per_view(), self.columns))
        per_view = max(1, (eight - one) // 7)
        n = max(1, int(self.WORKSPACE_BUDGET // per_view))
        if self.tile_capacity > 0:                      # fixed segments are addressed with 32-bit key offsets
            n = max(1, min(n, ((1 << 32) - 1) // (self.tiles * self.tile_capacity)))
        return n

    def _keys_per_view(self):
        return max(self.per_view_capacity, self.tiles * self.tile_capacity)

    def _workspace(self, nbytes, slot=0):
        """The workspace of `slot`, grown on demand and never shrunk.  Slot 0 is `launch`'s; "pose", "render" and "point" have one each,
        so the packed static records of `launch` stay where they are."""
        ws = self._ws.get(slot)
        if ws is None or ws.numel() < nbytes:
            self._ws[slot] = None
            ws = self._ws[slot] = torch.empty((nbytes,), dtype=torch.uint8, device=self.dev)
        return ws

    def _batch(self, w2c, poses_are_c2w):
        """What every batched launch starts with: (w2c [V,4,4] contiguous fp32 on the device, V, vis_count [V], num_rendered [V],
        status [4], max_rendered, a FisherCfg with the fields all four entry points share), the spatial order brought up to date."""
        d = self.dev
        w2c = _prep(w2c.reshape(-1, 4, 4), d)
        V = int(w2c.shape[0])
        # zero-filled / fully written by the library itself (k_zero_many, k_scan_tiles, k_reduce_scores): no fill kernels here
        vis = torch.empty((V,), dtype=torch.int32, device=d)
        nr = torch.empty((V,), dtype=torch.int32, device=d)
        status = torch.empty((4,), dtype=torch.int32, device=d)
        self._sync_order()
        fc = FisherCfg()
        fc.n_views, fc.columns, fc.dL_dpix = V, self.columns, self.dL
        fc.poses_are_c2w = 1 if poses_are_c2w else 0
        fc.tile_capacity = self.tile_capacity if V * self.tiles * self.tile_capacity < (1 << 32) else 0
        fc.w2c = ctypes.c_void_p(w2c.data_ptr())
        fc.out_vis_count = vis.data_ptr()
        fc.out_num_rendered = nr.data_ptr()
        fc.order = self.order.data_ptr() if self.order is not None else None
        return w2c, V, vis, nr, status, V * self._keys_per_view(), fc

    def _call(self, name, fc, outputs, ws, max_rendered, status):
        """One batched entry point of the library on this scorer's device and the current stream; `outputs`: the pointers it takes
        between the fisher cfg and the workspace."""
        with torch.cuda.device(self.dev):
            _lib.check(getattr(self.lib, name)(ctypes.byref(self.cfg), ctypes.byref(self.g), ctypes.byref(fc), *outputs,
                                               ws.data_ptr(), ws.numel(), max_rendered, status.data_ptr(), _stream(self.dev)), name)

    def _chunks(self, V, launch):
        """The launches that cover V views: `launch(v0, v1)` enqueues views [v0, v1) and returns the dict of its `*_launch` method;
        yields those dicts, one per chunk of at most `max_views_per_launch()` views.  One read of the 16-byte status word per
        attempt.  On overflow NOTHING was scored, accumulated or written (every kernel behind the scan returns on the overflow flag,
        include/fisher_rast.h), so outputs are as they were: the buffers grow and the chunk -- a shorter one where the larger
        buffers ask for it, which is why `launch` slices per call -- is redone.
        status[3]: bit 0 = a tile list longer than its fixed segment (k_tile_lists, every entry point), bit 1 = the camera's view
        matrix is not the identity `view_is_identity` promised (k_preprocess_views_c of fr_fisher_views alone: only `launch` sets
        the hint); nothing else is written there, the batched entry points clear `prefiltered`."""
        chunk = self.max_views_per_launch()
        v0 = 0
        while v0 < V:
            v1 = min(V, v0 + chunk)
            while True:
                r = launch(v0, v1)
                st = r["status"].cpu()
                if int(st[1]) == 0:
                    break
                if int(st[3]) & 2:
                    raise FisherRastError("FisherScorer.view_is_identity is set, but the camera's view matrix is not the identity "
                                          "(nothing was scored)")
                if int(st[3]) & 1:
                    # (st[2] = the longest list) longer segments, or packed lists
                    want = (int(int(st[2]) * 1.25) + 1023) // 1024 * 1024
                    self.tile_capacity = want if self.tiles * want * 8 <= self.MAX_KEY_BYTES_PER_VIEW else 0
                self.per_view_capacity = max(self.per_view_capacity, int(int(st[0]) * 1.25 / (v1 - v0)) + 4096)
                chunk = min(chunk, self.max_views_per_launch())
                v1 = min(v1, v0 + chunk)
            yield r
            v0 = v1

    def launch(self, w2c, H_inv=None, H_inv_per_view=False, out_H=None, out_H_per_view=False, dL_image=None, poses_are_c2w=False):
        """Enqueue one batch (no sync).  w2c: [V,4,4] world->camera on the device (camera->world with `poses_are_c2w`: the
        library inverts them).
        Returns a dict of device tensors: scores [V] (if H_inv), vis_count [V], num_rendered [V], status [4]."""
        d = self.dev
        # ONE fr_fisher_views call per launch: a call accumulates into out_H all or nothing (overflow: nothing), which is what lets
        # `run` simply redo a batch.  (Round 3 could cut a batch into view groups on separate streams; it measured slower -- 2.47 ms
        # against 2.08 ms per step -- and a group that had not overflowed would have been added to out_H twice by the redo.)
        w2c, V, vis, nr, status, max_rendered, fc = self._batch(w2c, poses_are_c2w)
        PC = self.P * self.columns
        scores = None
        if H_inv is not None:
            H_inv = _prep(H_inv, d)
            want = (V * PC) if H_inv_per_view else PC
            if H_inv.numel() != want:
                raise ValueError(f"H_inv has {H_inv.numel()} elements, expected {want}")
            scores = torch.empty((V,), dtype=torch.float32, device=d)     # every element is written (or the status word says overflow)
            fc.H_inv = ctypes.c_void_p(H_inv.data_ptr())
            fc.H_inv_view_stride = PC if H_inv_per_view else 0
            fc.out_scores = ctypes.c_void_p(scores.data_ptr())
        if out_H is not None:
            want = (V * PC) if out_H_per_view else PC
            if out_H.numel() != want or out_H.dtype != torch.float32 or not out_H.is_contiguous() or out_H.device != d:
                raise ValueError("out_H must be a contiguous fp32 device tensor of [V,]P*columns elements")
            fc.out_H = ctypes.c_void_p(out_H.data_ptr())
            fc.out_H_view_stride = PC if out_H_per_view else 0
        if dL_image is not None:
            # per view an upstream-gradient image [V,3,H,W] (or one [3,H,W] shared): the random probes of the POp-GS estimators
            if out_H is None or H_inv is not None:
                raise ValueError("dL_image goes with out_H (no H_inv)")
            HW3 = 3 * int(self.rs.image_height) * int(self.rs.image_width)
            dL_image = _prep(dL_image, d)
            if dL_image.numel() not in (HW3, V * HW3):
                raise ValueError(f"dL_image has {dL_image.numel()} elements, expected {HW3} or {V * HW3}")
            fc.dL_dpix_image = ctypes.c_void_p(dL_image.data_ptr())
            fc.dL_image_view_stride = HW3 if dL_image.numel() != HW3 else 0
        fc.view_is_identity = 1 if self.view_is_identity else 0
        nbytes = int(self.lib.fr_fisher_workspace_bytes(self.P, self.W, self.H, V, max_rendered, self.columns))
        if nbytes == 0:
            raise FisherRastError("fr_fisher_workspace_bytes: bad argument")
        ws = self._workspace(nbytes)
        # the per-Gaussian static records (means, cov3D, colours, shared H_inv rows) are packed into the workspace by every call; a call
        # that finds there what it would write -- same workspace and layout, same shared H_inv tensor in the same version, the map's
        # tensors (and the order) at the same addresses in the same versions -- skips that kernel (fr_fisher_cfg.reuse_static)
        # (the H_inv TENSOR is held on to: a fresh tensor of a later call can then not land on its address and pass for it)
        shared = None if (H_inv is None or H_inv_per_view) else H_inv
        skey = (ws.data_ptr(), ws.numel(), V, max_rendered, fc.tile_capacity, None if shared is None else shared._version, self._map_key())
        if H_inv is not None and out_H is not None:
            # scores AND diagonals in one call run the two-pass fall-back kernel, which packs its own static records and leaves the
            # front end's {mean, trace} array unwritten: nothing of this call may be reused by the next one
            skey = None
        fc.reuse_static = 1 if (skey is not None and self._static_key == skey and self._static_hinv is shared) else 0
        self._static_key, self._static_hinv = None, None            # (set again once the call has been enqueued without an error)
        self._call("fr_fisher_views", fc, (), ws, max_rendered, status)
        self._static_key, self._static_hinv = skey, shared
        return dict(scores=scores, vis_count=vis, num_rendered=nr, status=status, n_views=V, _keep=(w2c, H_inv, dL_image))

    def run(self, w2c, H_inv=None, H_inv_per_view=False, out_H=None, out_H_per_view=False, dL_image=None, poses_are_c2w=False):
        """launch() + overflow handling.  Synchronises once (to read the 16-byte status word)."""
        w2c = w2c.reshape(-1, 4, 4)
        V = int(w2c.shape[0])

        def launch(v0, v1):
            hi = H_inv.reshape(V, -1)[v0:v1] if (H_inv is not None and H_inv_per_view) else H_inv
            oh = out_H.view(V, -1)[v0:v1] if (out_H is not None and out_H_per_view) else out_H
            dl = dL_image[v0:v1] if (dL_image is not None and dL_image.dim() == 4 and dL_image.shape[0] == V) else dL_image
            return self.launch(w2c[v0:v1], hi, H_inv_per_view, oh, out_H_per_view, dl, poses_are_c2w)
        outs = list(self._chunks(V, launch))
        res = dict(vis_count=torch.cat([o["vis_count"] for o in outs]),
                   num_rendered=torch.cat([o["num_rendered"] for o in outs]))
        res["scores"] = torch.cat([o["scores"] for o in outs]) if H_inv is not None else None
        return res

    # -- camera-pose Fisher information (fr_fisher_pose_views) ---------------------------------------------
    def pose_launch(self, w2c, poses_are_c2w=False, out=None):
        """Enqueue one batch of pose Fisher matrices (no sync).  Returns a dict of device tensors: pose_H [V,6,6] (`out` when given:
        a contiguous fp32 device tensor of 36 V elements), vis_count [V], num_rendered [V], status [4].  Its own workspace: the packed
        static records of `launch` stay where they are."""
        d = self.dev
        w2c, V, vis, nr, status, max_rendered, fc = self._batch(w2c, poses_are_c2w)
        if out is not None and (out.numel() != 36 * V or out.dtype != torch.float32 or not out.is_contiguous() or out.device != d):
            raise ValueError("out must be a contiguous fp32 device tensor of V*36 elements")
        # every element is written (or the status word says overflow, and none is)
        pose_H = out.view(V, 6, 6) if out is not None else torch.empty((V, 6, 6), dtype=torch.float32, device=d)
        nbytes = int(self.lib.fr_fisher_pose_workspace_bytes(self.P, self.W, self.H, V, max_rendered))
        if nbytes == 0:
            raise FisherRastError("fr_fisher_pose_workspace_bytes: bad argument")
        self._call("fr_fisher_pose_views", fc, (ctypes.c_void_p(pose_H.data_ptr()),), self._workspace(nbytes, "pose"), max_rendered, status)
        return dict(pose_H=pose_H, vis_count=vis, num_rendered=nr, status=status, n_views=V, _keep=(w2c,))

    def pose_fisher(self, w2c, poses_are_c2w=False):
        """Camera-pose Fisher information of every view: [V,6,6] float32 on the device, xi = (translation, rotation), left
        perturbation of the camera-frame means (include/fisher_rast.h, fr_fisher_pose_views).  Views beyond
        `max_views_per_launch()` go in several calls; an overflow of the key buffer is redone with a larger one, as in `run`.
        Synchronises once per call (the status word).  The same for 4- and 11-column scorers."""
        w2c = w2c.reshape(-1, 4, 4)
        outs = [r["pose_H"] for r in self._chunks(int(w2c.shape[0]), lambda v0, v1: self.pose_launch(w2c[v0:v1], poses_are_c2w))]
        return torch.cat(outs) if outs else torch.zeros((0, 6, 6), dtype=torch.float32, device=self.dev)

    # -- batched render of candidate views (fr_render_views) -----------------------------------------------
    def render_launch(self, w2c, poses_are_c2w=False, features=True, depth=True, final_T=True, render=True, out=None):
        """Enqueue one batch of renders (no sync).  Returns a dict of device tensors: render [V,3,H,W], depth_sil [V,3,H,W] (the
        composited (z, 1, z z) of the camera-frame depth; `features`), median_depth [V,1,H,W] (`depth`), final_T [V,H,W], each None
        when not asked for, and vis_count [V], num_rendered [V], status [4].  On overflow (status[1]) no image byte is written.
        `out`: a dict that may hold contiguous fp32 device tensors of those shapes under those four names, written instead of fresh ones.
        Its own workspace, as `pose_launch`: the packed static records of `launch` stay where they are."""
        d = self.dev
        w2c, V, vis, nr, status, max_rendered, fc = self._batch(w2c, poses_are_c2w)       # (columns and dL_dpix are set too: the library ignores them here)
        H, W = self.H, self.W
        if not (render or features or depth or final_T):
            raise ValueError("render_launch: no output requested")

        given = out or {}

        def new(name, *shape):                              # every element is written (or the status word says overflow, and none is)
            t = given.get(name)
            if t is None:
                return torch.empty(shape, dtype=torch.float32, device=d)
            if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != d:
                raise ValueError(f"out['{name}'] must be a contiguous fp32 device tensor of shape {shape}")
            return t
        out = dict(render=new("render", V, 3, H, W) if render else None, depth_sil=new("depth_sil", V, 3, H, W) if features else None,
                   median_depth=new("median_depth", V, 1, H, W) if depth else None, final_T=new("final_T", V, H, W) if final_T else None)
        nbytes = int(self.lib.fr_render_views_workspace_bytes(self.P, W, H, V, max_rendered))
        if nbytes == 0:
            raise FisherRastError("fr_render_views_workspace_bytes: bad argument (or an image beyond 4096 tiles: render_views loops there)")
        self._call("fr_render_views", fc, (_ptr(out["render"]), _ptr(out["depth_sil"]), _ptr(out["median_depth"]), _ptr(out["final_T"])),
                   self._workspace(nbytes, "render"), max_rendered, status)
        out.update(vis_count=vis, num_rendered=nr, status=status, n_views=V, _keep=(w2c,))
        return out

    @staticmethod
    def _invert_poses(m):
        """The library's pose inverse (k_invert_poses) restated in float64 elementwise ops on the host: the adjugate by cofactor
        expansion, times 1 / det, rounded once to float -- the same products and sums in the same order, so the same bits."""
        dev = m.device
        m = m.detach().cpu().double().reshape(-1, 16)
        m = [m[:, k] for k in range(16)]
        inv = [None] * 16
        inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10]
        inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10]
        inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9]
        inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9]
        inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10]
        inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10]
        inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9]
        inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9]
        inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6]
        inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6]
        inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5]
        inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5]
        inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6]
        inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6]
        inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5]
        inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5]
        det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]
        r = 1.0 / det
        return torch.stack([x * r for x in inv], dim=1).float().reshape(-1, 4, 4).to(dev)

    def _render_views_serial(self, w2c, poses_are_c2w, features, depth, final_T):
        """Images beyond 4096 tiles: view after view through the single-view rasteriser (`rasterize_forward`, the pair path).  The
        camera-frame means are formed in torch elementwise ops in the order the library uses, ((w0 x + w1 y) + w2 z) + w3, each
        product and sum rounded on its own, and camera-to-world poses are inverted as the library inverts them (`_invert_poses`),
        so the images are the ones `fr_render_views` would give."""
        d = self.dev
        w2c = _prep(w2c.reshape(-1, 4, 4), d)
        if poses_are_c2w:
            w2c = self._invert_poses(w2c)
        rs = self.rs
        x, y, z = self.means3D[:, 0], self.means3D[:, 1], self.means3D[:, 2]
        empty = torch.Tensor([])
        outs = dict(render=[], depth_sil=[], median_depth=[], final_T=[], vis_count=[], num_rendered=[])
        for w in w2c:
            rows = []
            for r in range(3):
                t = torch.mul(x, w[r, 0]) + torch.mul(y, w[r, 1])
                t = t + torch.mul(z, w[r, 2])
                rows.append(t + w[r, 3])
            m = torch.stack(rows, dim=1)
            feats = torch.stack((m[:, 2], torch.ones_like(m[:, 2]), m[:, 2] * m[:, 2]), dim=1)
            res = rasterize_forward(self.bg, m, self.colors, self.opacities, self.scales, self.rotations, rs.scale_modifier, empty,
                                    self.view, self.proj, rs.tanfovx, rs.tanfovy, self.H, self.W, empty, rs.sh_degree, self.campos,
                                    False, features=feats if features else None)
            nr, color, radii, img = res[0], res[1], res[2], res[5]
            outs["render"].append(color)
            outs["median_depth"].append(res[6])
            if features:
                outs["depth_sil"].append(res[7])
            if final_T:
                off = workspace_layout(self.P, self.W, self.H, 1)["final_T"]
                outs["final_T"].append(img[off:off + 4 * self.H * self.W].view(torch.float32).reshape(self.H, self.W).clone())
            outs["vis_count"].append((radii > 0).sum().to(torch.int32).reshape(1))
            outs["num_rendered"].append(torch.tensor([nr], dtype=torch.int32, device=d))
        return dict(render=torch.stack(outs["render"]), depth_sil=torch.stack(outs["depth_sil"]) if features else None,
                    median_depth=torch.stack(outs["median_depth"]) if depth else None,
                    final_T=torch.stack(outs["final_T"]) if final_T else None,
                    vis_count=torch.cat(outs["vis_count"]), num_rendered=torch.cat(outs["num_rendered"]))

    def render_views(self, w2c, poses_are_c2w=False, features=True, depth=True, final_T=True):
        """RGB, depth / silhouette, median depth and final transmittance of every view: what the single-view rasteriser gives for the
        camera-frame means of the view, bit for bit (include/fisher_rast.h, fr_render_views).  Returns dict(render [V,3,H,W],
        depth_sil [V,3,H,W], median_depth [V,1,H,W], final_T [V,H,W], vis_count [V], num_rendered [V]) on the device; the optional
        ones are None when switched off.  Views beyond `max_views_per_launch()` go in several calls; an overflow of the key buffer is
        redone with a larger one, as in `pose_fisher`: one status read per chunk.  Images beyond 4096 tiles: a loop of single-view
        renders."""
        w2c = w2c.reshape(-1, 4, 4)
        V = int(w2c.shape[0])
        if self.tiles > 4096:
            return self._render_views_serial(w2c, poses_are_c2w, features, depth, final_T)
        outs = list(self._chunks(V, lambda v0, v1: self.render_launch(w2c[v0:v1], poses_are_c2w, features, depth, final_T)))
        names = ("render", "depth_sil", "median_depth", "final_T", "vis_count", "num_rendered")
        if len(outs) == 1:
            return {k: outs[0][k] for k in names}
        if not outs:
            H, W = self.H, self.W
            shapes = dict(render=(0, 3, H, W), depth_sil=(0, 3, H, W), median_depth=(0, 1, H, W), final_T=(0, H, W))
            on = dict(render=True, depth_sil=features, median_depth=depth, final_T=final_T)
            res = {k: torch.zeros(shapes[k], dtype=torch.float32, device=self.dev) if on[k] else None for k in shapes}
            res.update(vis_count=torch.zeros((0,), dtype=torch.int32, device=self.dev), num_rendered=torch.zeros((0,), dtype=torch.int32, device=self.dev))
            return res
        return {k: (torch.cat([o[k] for o in outs]) if outs[0][k] is not None else None) for k in names}


    # -- per-Gaussian view scores and their running maximum (fr_fisher_point_views) -----------------------
    def point_launch(self, w2c, H_inv, H_inv_per_view=False, per_view=True, out=None, point_max=None, poses_are_c2w=False):
        """Enqueue one batch of per-Gaussian view scores (no sync): point[v, i] = sum_c cur_H[v, i, c] H_inv[(v,) i, c], the
        `pointScores` of the reference's candidate scan (models/SLAM/gaussian.py:1285-1325), without a [V, P, columns] tensor.
        Returns a dict of device tensors: point_scores [V,P] (`per_view`; `out` when given), point_max [P] (`point_max` when given --
        the running maximum is taken INTO it, so it composes over calls; a fresh one starts from zeros, as the reference does),
        scores [V], vis_count [V], num_rendered [V], status [4].  On overflow (status[1]) no output byte is written.
        Its own workspace, as `pose_launch`: the packed static records of `launch` stay where they are."""
        d = self.dev
        w2c, V, vis, nr, status, max_rendered, fc = self._batch(w2c, poses_are_c2w)
        P, PC = self.P, self.P * self.columns
        if H_inv is None:
            raise ValueError("point_launch needs H_inv")
        want = (V * PC) if H_inv_per_view else PC
        if H_inv.numel() != want:
            raise ValueError(f"H_inv has {H_inv.numel()} elements, expected {want}")
        H_inv = _prep(H_inv, d)

        def given(t, n, name):
            if t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() or t.device != d:
                raise ValueError(f"{name} must be a contiguous fp32 device tensor of {n} elements")
            return t
        point = None
        if out is not None:
            point = given(out, V * P, "out").view(V, P)
        elif per_view:
            point = torch.empty((V, P), dtype=torch.float32, device=d)        # every element is written (or the status word says overflow)
        pmax = given(point_max, P, "point_max") if point_max is not None else torch.zeros((P,), dtype=torch.float32, device=d)
        scores = torch.empty((V,), dtype=torch.float32, device=d)
        nbytes = int(self.lib.fr_fisher_point_workspace_bytes(P, self.W, self.H, V, max_rendered, self.columns))
        if nbytes == 0:
            raise FisherRastError("fr_fisher_point_workspace_bytes: bad argument (or an image beyond 4096 tiles)")
        fc.H_inv = ctypes.c_void_p(H_inv.data_ptr())
        fc.H_inv_view_stride = PC if H_inv_per_view else 0
        fc.out_scores = ctypes.c_void_p(scores.data_ptr())
        self._call("fr_fisher_point_views", fc, (_ptr(point), _ptr(pmax)), self._workspace(nbytes, "point"), max_rendered, status)
        return dict(point_scores=point, point_max=pmax, scores=scores, vis_count=vis, num_rendered=nr, status=status, n_views=V,
                    _keep=(w2c, H_inv))

    def point_scores(self, w2c, H_inv, H_inv_per_view=False, per_view=True, point_max=None, poses_are_c2w=False):
        """Per-Gaussian scores of every view and their maximum over the views (include/fisher_rast.h, fr_fisher_point_views).
        Returns dict(scores [V], point_max [P], point_scores [V,P] (when `per_view`), vis_count [V], num_rendered [V]) on the device.
        `point_max`: a [P] fp32 device tensor of non-negative values to take the maximum into (default: zeros).  Views beyond
        `max_views_per_launch()` go in several calls into the same maximum; an overflow of the key buffer is redone with a larger one,
        as in `pose_fisher` (nothing was written): one status read per chunk."""
        d = self.dev
        w2c = w2c.reshape(-1, 4, 4)
        V, P = int(w2c.shape[0]), self.P
        if point_max is None:
            point_max = torch.zeros((P,), dtype=torch.float32, device=d)
        point = torch.empty((V, P), dtype=torch.float32, device=d) if per_view else None

        def launch(v0, v1):
            hi = H_inv.reshape(V, -1)[v0:v1] if H_inv_per_view else H_inv
            return self.point_launch(w2c[v0:v1], hi, H_inv_per_view, per_view, point[v0:v1] if per_view else None, point_max, poses_are_c2w)
        outs = list(self._chunks(V, launch))

        def cat(k, dtype):
            return torch.cat([o[k] for o in outs]) if outs else torch.zeros((0,), dtype=dtype, device=d)
        res = dict(scores=cat("scores", torch.float32), point_max=point_max, vis_count=cat("vis_count", torch.int32),
                   num_rendered=cat("num_rendered", torch.int32))
        if per_view:
            res["point_scores"] = point
        return res

    # -- POp-GS block stage (fr_raster_cfg.ext: fr_fisher_views renders nothing, include/fisher_rast.h) -------------------------
    def _block_stage(self, ext, w2cs, K, rows=None):
        """One call of the block stage on the current stream (no sync): `ext` filled by the caller, poses w2cs [V,4,4] (each repeated
        per probe here, as the C side reads pose p from view p K), rows [V,K,P,11] or None.  Returns the status word [4] (device)."""
        d = self.dev
        if self.P == 0:
            raise FisherRastError("the POp-GS block stage needs a map of at least one Gaussian")
        w2cs = _prep(w2cs.reshape(-1, 4, 4), d)
        V, K = int(w2cs.shape[0]), int(K)
        views = w2cs.repeat_interleave(K, dim=0).contiguous() if K > 1 else w2cs
        if rows is not None and (rows.numel() != V * K * self.P * 11 or rows.dtype != torch.float32 or not rows.is_contiguous() or rows.device != d):
            raise ValueError("rows must be a contiguous fp32 device tensor [V, K, P, 11]")
        ext.kind, ext.K = _lib.FR_EXT_POPGS_BLOCK, K
        cfg = RasterCfg.from_buffer_copy(self.cfg)
        cfg.ext = ctypes.pointer(ext)
        fc = FisherCfg()
        fc.n_views, fc.columns = V * K, 11
        fc.w2c = ctypes.c_void_p(views.data_ptr())
        fc.out_H = None if rows is None else ctypes.c_void_p(rows.data_ptr())
        fc.out_H_view_stride = 11 * self.P
        ws = self._workspace(_lib.popgs_block_workspace_bytes(self.P, V), "block")
        status = torch.empty((4,), dtype=torch.int32, device=d)
        with torch.cuda.device(d):
            _lib.check(self.lib.fr_fisher_views(ctypes.byref(cfg), ctypes.byref(self.g), ctypes.byref(fc), ws.data_ptr(), ws.numel(), 0,
                                                status.data_ptr(), _stream(d)), "fr_fisher_views (POp-GS block stage)")
        return status

    @staticmethod
    def _block_flags(ext, use_rot, use_scale, use_opacity):
        ext.use_rot, ext.use_scale, ext.use_opacity = int(bool(use_rot)), int(bool(use_scale)), int(bool(use_opacity))
        return _lib.popgs_block_dim(use_opacity, use_rot, use_scale)

    def visible(self, w2cs):
        """(mask bool [V,P], counts int32 [V]) on the device: Gaussian i has radius > 0 at pose v -- the single-view rasteriser's
        `radii > 0`, bit for bit, without rendering.  No sync."""
        d = self.dev
        V = int(w2cs.reshape(-1, 4, 4).shape[0])
        mask = torch.empty((V, self.P), dtype=torch.uint8, device=d)
        counts = torch.empty((V,), dtype=torch.int32, device=d)
        if V == 0 or self.P == 0:
            return mask.view(torch.bool), counts.zero_()
        ext = _lib.RasterExt()
        ext.mode, ext.out_vis, ext.out_vis_count = _lib.FR_POPGS_BLOCK_VISIBLE, mask.data_ptr(), counts.data_ptr()
        self._block_stage(ext, w2cs, 1)
        return mask.view(torch.bool), counts

    def popgs_block_prior(self, rows, w2cs, K, use_rot=True, use_scale=True, use_opacity=True):
        """compute_H_train_blocks from the keyframes' probe rows [V,K,P,11] and poses w2cs [V,4,4], the reference's truncation kept:
        (Hm [n,d,d] fp32, idx [n] int32), n = the smallest visible count.  One host read (n)."""
        d = self.dev
        ext = _lib.RasterExt()
        dim = self._block_flags(ext, use_rot, use_scale, use_opacity)
        Hm = torch.empty((self.P, dim, dim), dtype=torch.float32, device=d)
        idx = torch.empty((self.P,), dtype=torch.int32, device=d)
        ext.mode, ext.n, ext.prior_blocks, ext.prior_idx = _lib.FR_POPGS_BLOCK_PRIOR, self.P, Hm.data_ptr(), idx.data_ptr()
        status = self._block_stage(ext, w2cs, K, rows)
        n = int(status[0].item())
        return Hm[:n], idx[:n]

    def popgs_block_scores(self, rows, w2cs, K, Hm, idx, lam=1e-6, criterion="topt", use_rot=True, use_scale=True, use_opacity=True, vis=None):
        """Block T-opt / D-opt scores of V poses from their probe rows [V,K,P,11] against the prior (Hm [n,d,d], idx [n]):
        (scores float64 [V], matched int32 [V]) on the device, no sync; a pose that sees none of the prior's Gaussians scores -inf.
        `vis` (bool / uint8 [V,P]) replaces the visibility the call would compute from w2cs.  The status word of the call
        ({pairs, 0, non-positive pivots, prior rows with an index outside the map}) is left in `self.block_status`."""
        d = self.dev
        if criterion not in ("topt", "dopt"):
            raise ValueError("criterion must be 'topt' or 'dopt'")
        V = int(w2cs.reshape(-1, 4, 4).shape[0])
        scores = torch.empty((V,), dtype=torch.float64, device=d)
        matched = torch.empty((V,), dtype=torch.int32, device=d)
        ext = _lib.RasterExt()
        dim = self._block_flags(ext, use_rot, use_scale, use_opacity)
        n = int(idx.shape[0])
        if tuple(Hm.shape) != (n, dim, dim):
            raise ValueError(f"Hm is {tuple(Hm.shape)}, expected {(n, dim, dim)}")
        if n == 0 or V == 0:
            self.block_status = torch.zeros((4,), dtype=torch.int32, device=d)
            return scores.fill_(float("-inf")), matched.zero_()
        Hm = _prep(Hm, d)
        idx = idx.to(device=d, dtype=torch.int32).contiguous()
        if vis is not None:
            if tuple(vis.shape) != (V, self.P) or vis.dtype not in (torch.bool, torch.uint8):
                raise ValueError("vis must be bool or uint8 [V, P]")
            vis = vis.to(d).contiguous().view(torch.uint8)
            ext.vis_in = vis.data_ptr()
        ext.mode, ext.n, ext.lam = _lib.FR_POPGS_BLOCK_SCORE, n, float(lam)
        ext.criterion = _lib.FR_POPGS_TOPT if criterion == "topt" else _lib.FR_POPGS_DOPT
        ext.prior_blocks, ext.prior_idx, ext.out_scores, ext.out_matched = Hm.data_ptr(), idx.data_ptr(), scores.data_ptr(), matched.data_ptr()
        self.block_status = self._block_stage(ext, w2cs, K, rows)
        return scores, matched


def spatial_order_of(means3D: torch.Tensor) -> torch.Tensor:
    """fr_spatial_order: int32 [P], entry k = index of the k-th Gaussian along the Z-curve of the means (stable for equal codes)."""
    _need_gpu(means3D, "means3D")
    dev = means3D.device
    lib = _lib.load()
    pts = _prep(means3D.detach(), dev)
    P = int(pts.shape[0]) if pts is not None else 0
    if P == 0:
        return torch.zeros((0,), dtype=torch.int32, device=dev)
    order = torch.empty((P,), dtype=torch.int32, device=dev)
    ws = torch.empty((max(int(lib.fr_spatial_order_workspace_bytes(P)), 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_spatial_order(P, _ptr(pts), order.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)), "fr_spatial_order")
    return order


def knn_dist2(points: torch.Tensor) -> torch.Tensor:
    """simple_knn._C.distCUDA2: mean squared distance to the 3 nearest other points, [P,3] -> [P]."""
    _need_gpu(points, "points")
    dev = points.device
    lib = _lib.load()
    pts = _prep(points, dev)
    P = int(pts.shape[0]) if pts is not None else 0
    if P == 0:
        return torch.zeros((0,), dtype=torch.float32, device=dev)
    out = torch.empty((P,), dtype=torch.float32, device=dev)          # k_knn_search writes every element: no fill kernel in front of it
    nbytes = int(lib.fr_knn_workspace_bytes(P))
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_knn_dist2(P, _ptr(pts), _ptr(out), ws.data_ptr(), ws.numel(), _stream(dev)), "fr_knn_dist2")
    return out


def popgs_diag_criterion(rows: torch.Tensor, prior_in: torch.Tensor, lam: float = 1e-6, criterion: str = "topt", *,
                         prior_out: Optional[torch.Tensor] = None, accumulate: Optional[torch.Tensor] = None,
                         vis_count: Optional[torch.Tensor] = None, scores: Optional[torch.Tensor] = None,
                         workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fr_popgs_diag_criterion: the POp-GS T-opt / D-opt score of V views from their probe rows, and optionally the views' updated
    priors, in one pass (tester_gaussians_navigation.py:2147-2178).
      rows [V, K, ...]   fp32 probe rows (`_pose_probe_rows`), E = the elements of one probe
      prior_in           E elements (shared by all views) or V * E (one block per view), in the layout of the rows
      prior_out          V * E elements or None; may be `prior_in` itself.  accumulate [V] (bool / uint8) says which views' blocks
                         receive prior_in + J; the others are left as they are
      vis_count [V]      int32 or None: a view that sees nothing scores exactly 0
    Returns scores [V] float64 on the device (no host synchronisation).  Nothing is copied or converted: tensors that are not
    contiguous fp32 (int32 / uint8 for the two small ones) on the device of `rows` are an error."""
    _need_gpu(rows, "rows")
    dev = rows.device
    if rows.dim() < 3:
        raise FisherRastError("rows must be [V, K, ...]")
    V, K = int(rows.shape[0]), int(rows.shape[1])
    E = rows.numel() // max(V * K, 1)
    crit = {"topt": _lib.FR_POPGS_TOPT, "dopt": _lib.FR_POPGS_DOPT}.get(str(criterion).lower())
    if crit is None:
        raise ValueError("criterion must be 'topt' or 'dopt'")

    def plain(t, name, dtype):
        _need_gpu(t, name)
        if t.device != dev or t.dtype != dtype or not t.is_contiguous():
            raise FisherRastError(f"{name} must be a contiguous {dtype} tensor on {dev}")
        return t

    plain(rows, "rows", torch.float32)
    plain(prior_in, "prior_in", torch.float32)
    if prior_in.numel() not in (E, V * E):
        raise FisherRastError(f"prior_in has {prior_in.numel()} elements, expected {E} (shared) or {V * E} (per view)")
    stride = E if prior_in.numel() == V * E and V > 1 else 0
    if prior_out is not None and plain(prior_out, "prior_out", torch.float32).numel() != V * E:
        raise FisherRastError(f"prior_out has {prior_out.numel()} elements, expected {V * E}")
    if accumulate is not None:
        accumulate = torch.as_tensor(accumulate)
        if accumulate.dtype == torch.bool:
            accumulate = accumulate.to(torch.uint8)
        if not accumulate.is_cuda:
            accumulate = accumulate.to(dev)
        if plain(accumulate, "accumulate", torch.uint8).numel() != V:
            raise FisherRastError("accumulate must have one entry per view")
        if prior_out is None:
            raise FisherRastError("accumulate needs prior_out")
    if vis_count is not None and plain(vis_count, "vis_count", torch.int32).numel() != V:
        raise FisherRastError("vis_count must have one entry per view")
    lib = _lib.load()
    need = int(lib.fr_popgs_diag_criterion_workspace_bytes(V, E))
    if workspace is None:
        workspace = torch.empty((max(need, 8) // 8,), dtype=torch.float64, device=dev)
    else:
        plain(workspace, "workspace", workspace.dtype)
    if scores is None:
        scores = torch.empty((V,), dtype=torch.float64, device=dev)
    elif plain(scores, "scores", torch.float64).numel() != V:
        raise FisherRastError("scores must have one entry per view")
    with torch.cuda.device(dev):
        _lib.check(lib.fr_popgs_diag_criterion(V, K, E, _ptr(rows), _ptr(prior_in), stride, _ptr(prior_out), _ptr(accumulate),
                                               _ptr(vis_count), float(lam), crit, _ptr(scores), _ptr(workspace),
                                               workspace.numel() * workspace.element_size(), _stream(dev)),
                   "fr_popgs_diag_criterion")
    return scores


def _small_f32(t, dev, rows, cols, name):
    """a [rows, cols] matrix (tensor on any device, array or nested list) as contiguous fp32 on `dev`, without a host
    synchronisation: a device tensor is used where it is; host values are staged in pinned memory and sent with a non-blocking
    copy (the host allocator keeps a pinned block until the copies issued from it have run, so dropping the staging tensor on
    return is safe)"""
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t, dtype=torch.float32)
    if t.dim() != 2 or t.shape[0] < rows or t.shape[1] < cols:
        raise FisherRastError(f"{name} must be at least [{rows},{cols}], got {tuple(t.shape)}")
    t = t[:rows, :cols]
    if t.device != dev:
        if t.is_cuda:
            return t.to(dev).float().contiguous()
        t = t.float().contiguous().pin_memory().to(dev, non_blocking=True)
    return t.float().contiguous()


def _ingest_plain(t, name, dev, dtype, shape):
    _need_gpu(t, name)
    if t.device != dev or t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise FisherRastError(f"{name} must be a contiguous {dtype} tensor of {tuple(shape)} on {dev}, got {t.dtype} {tuple(t.shape)}")
    return t


def frame_ingest_workspace(H, W, downsample, dev):
    need = int(_lib.load().fr_frame_ingest_workspace_bytes(int(H), int(W), int(downsample)))
    if need == 0:
        raise FisherRastError(f"frame ingest: downsample {downsample} must be positive and divide H = {H} and W = {W}")
    return torch.empty(((need + 7) // 8,), dtype=torch.int64, device=dev)


def _mask_bytes_hw(mask, H, W, name):
    """a [H,W] mask (bool / uint8, or anything compared with 0) as contiguous bytes; bool is reinterpreted, not copied"""
    _need_gpu(mask, name)
    if mask.numel() != H * W:
        raise FisherRastError(f"frame ingest: {name} of {tuple(mask.shape)} does not fit a frame of {H} x {W}")
    m = mask if mask.dtype in (torch.bool, torch.uint8) else (mask != 0)
    m = m.contiguous()
    return m.view(torch.uint8) if m.dtype == torch.bool else m


def frame_ingest_select(depth_sil=None, gt_depth=None, mask=None, *, and_mask=None, downsample=1, sil_thres=0.5, depth_error_ratio=50.0,
                        workspace=None, status=None):
    """fr_frame_ingest_select.  With `mask` (bool / uint8, H W elements, given together with its [*,H,W] shaped `gt_depth` or
    `depth_sil` for the size, or itself [H,W]) the caller's mask is pooled and compacted; without, the non-presence mask is built
    from depth_sil [3,H,W] (depth, silhouette, ..) and gt_depth [1,H,W], ANDed with `and_mask` (H W elements; the object
    mask of the object-aware SLAM class) where one is given.  Returns (status, workspace): status int32
    [FR_INGEST_STATUS_WORDS] on the device = {count, median is NaN, 0, 0, median bits} -- reading it is the caller's one host
    synchronisation -- and the workspace that holds the index list for `frame_ingest_emit`.  No host synchronisation in here."""
    ref = gt_depth if gt_depth is not None else (depth_sil if depth_sil is not None else mask)
    if ref is None:
        raise FisherRastError("frame ingest: nothing to select from")
    _need_gpu(ref, "frame ingest input")
    dev = ref.device
    H, W = int(ref.shape[-2]), int(ref.shape[-1])
    cfg = FrameIngestCfg(H, W, int(downsample), _lib.FR_INGEST_NONPRESENCE if mask is None else _lib.FR_INGEST_MASK,
                         float(sil_thres), float(depth_error_ratio), 1, 3, 3, 3, None)
    if mask is None:
        _ingest_plain(depth_sil, "depth_sil", dev, torch.float32, (3, H, W))
        _ingest_plain(gt_depth, "gt_depth", dev, torch.float32, (1, H, W))
        m = None if and_mask is None else _mask_bytes_hw(and_mask, H, W, "and_mask")
    else:
        if and_mask is not None:
            raise FisherRastError("frame ingest: and_mask goes with the non-presence mask, not with a caller's mask")
        m = _mask_bytes_hw(mask, H, W, "mask")
    if workspace is None:
        workspace = frame_ingest_workspace(H, W, downsample, dev)
    if status is None:
        status = torch.empty((_lib.FR_INGEST_STATUS_WORDS,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_frame_ingest_select(ctypes.byref(cfg), _ptr(depth_sil if mask is None else None),
                                                      _ptr(gt_depth if mask is None else None), _ptr(m), _ptr(status), _ptr(workspace),
                                                      workspace.numel() * workspace.element_size(), _stream(dev)),
                   "fr_frame_ingest_select")
    return status, workspace


def frame_ingest_emit(color, gt_depth, intrinsics, w2c, workspace, count, *, downsample=1, transform_pts=True, row_offset=0,
                      means3D=None, rgb_colors=None, unnorm_rotations=None, logit_opacities=None, log_scales=None, mean3_sq_dist=None,
                      point_cld=None):
    """fr_frame_ingest_emit: rows [row_offset, row_offset + count) of every destination given (contiguous fp32 on the device of
    `color`; `point_cld` [N,6] takes the point and the colour of a row side by side, in place of means3D and rgb_colors).
    workspace None with count == (H/d)(W/d): every cell.  intrinsics [3,3] and w2c [4,4] may live anywhere; on the device they are
    read where they are.  No host synchronisation."""
    _need_gpu(color, "color")
    dev = color.device
    H, W = int(color.shape[-2]), int(color.shape[-1])
    _ingest_plain(color, "color", dev, torch.float32, (3, H, W))
    _ingest_plain(gt_depth, "gt_depth", dev, torch.float32, (1, H, W))
    count, row_offset = int(count), int(row_offset)
    rows = row_offset + count
    K = _small_f32(intrinsics, dev, 3, 3, "intrinsics")
    pose = _small_f32(w2c, dev, 4, 4, "w2c") if transform_pts else None
    means_ptr, rgb_ptr, stride = _ptr(means3D), _ptr(rgb_colors), 3
    if point_cld is not None:
        if means3D is not None or rgb_colors is not None:
            raise FisherRastError("frame ingest: point_cld takes the place of means3D and rgb_colors")
        _ingest_plain(point_cld, "point_cld", dev, torch.float32, (point_cld.shape[0], 6))
        means_ptr, rgb_ptr, stride = ctypes.c_void_p(point_cld.data_ptr()), ctypes.c_void_p(point_cld.data_ptr() + 12), 6
    scale_cols = 3
    for t, name, cols in ((means3D, "means3D", 3), (rgb_colors, "rgb_colors", 3), (unnorm_rotations, "unnorm_rotations", 4),
                          (logit_opacities, "logit_opacities", 1), (log_scales, "log_scales", None), (mean3_sq_dist, "mean3_sq_dist", 0),
                          (point_cld, "point_cld", 6)):
        if t is None:
            continue
        if name == "log_scales":
            cols = scale_cols = int(t.shape[1]) if t.dim() == 2 else -1
        _ingest_plain(t, name, dev, torch.float32, (t.shape[0], cols) if cols else (t.shape[0],))
        if t.shape[0] < rows:
            raise FisherRastError(f"frame ingest: {name} has {t.shape[0]} rows, {rows} are written")
    cfg = FrameIngestCfg(H, W, int(downsample), 0, 0.0, 0.0, int(bool(transform_pts)), scale_cols, stride, stride, K.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_frame_ingest_emit(ctypes.byref(cfg), _ptr(color), _ptr(gt_depth), _ptr(pose), _ptr(workspace), count, row_offset,
                                                    means_ptr, rgb_ptr, _ptr(unnorm_rotations), _ptr(logit_opacities), _ptr(log_scales),
                                                    _ptr(mean3_sq_dist), _stream(dev)),
                   "fr_frame_ingest_emit")


# ---- keyframe overlap (fr_keyframe_valid_pixels / fr_keyframe_overlap) ----------------------------------------------------------------

_keyframe_ws = {}


def _keyframe_workspace(kind, shape, dev, nbytes):
    """the workspace of one of the two keyframe calls, kept per (device, stream) and shape, as `_backward_scratch` is: calls on one
    stream follow each other, calls on two streams may run side by side and get a workspace each"""
    key = (kind, dev, int(torch.cuda.current_stream(dev).cuda_stream), shape)
    ws = _keyframe_ws.get(key)
    if ws is None:
        if nbytes == 0:
            raise FisherRastError(f"keyframe overlap: bad size {shape}")
        ws = _keyframe_ws[key] = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    return ws


def _host_i64_to(values, dev):
    """int64 values (a host tensor or a list) on `dev` without a host synchronisation: staged in pinned memory (see _small_f32);
    a tensor already on the device is used where it is"""
    t = values if isinstance(values, torch.Tensor) else torch.tensor(values, dtype=torch.int64)
    if t.dtype != torch.int64:
        t = t.long()
    if t.device == dev:
        return t.contiguous()
    if t.is_cuda:
        return t.to(dev).contiguous()
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def _depth_hw(depth):
    _need_gpu(depth, "depth")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if depth.dtype != torch.float32 or not depth.is_contiguous() or depth.numel() != H * W:
        raise FisherRastError(f"keyframe overlap: depth must be a contiguous float32 [H,W] or [1,H,W] tensor, got {depth.dtype} {tuple(depth.shape)}")
    return H, W


def keyframe_valid_pixels(depth, mask=None, *, idx=None, status=None):
    """fr_keyframe_valid_pixels: (idx, status) -- idx int32 [H W] on the device, whose first status[0] entries are the ascending flat
    indices of depth > 0 (and mask != 0 where a mask of H W elements is given): the rows of torch.where in order.  status int32
    [FR_KEYFRAME_STATUS_WORDS] = {count, 0, 0, 0}; reading it is the caller's host synchronisation, there is none in here."""
    H, W = _depth_hw(depth)
    dev = depth.device
    m = None if mask is None else _mask_bytes_hw(mask, H, W, "mask")
    lib = _lib.load()
    ws = _keyframe_workspace("pixels", (H, W), dev, int(lib.fr_keyframe_valid_pixels_workspace_bytes(H, W)))
    if idx is None:
        idx = torch.empty((H * W,), dtype=torch.int32, device=dev)
    if status is None:
        status = torch.empty((_lib.FR_KEYFRAME_STATUS_WORDS,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_keyframe_valid_pixels(H, W, _ptr(depth), _ptr(m), _ptr(idx), _ptr(status), _ptr(ws),
                                                ws.numel() * ws.element_size(), _stream(dev)), "fr_keyframe_valid_pixels")
    return idx, status


def keyframe_overlap(depth, intrinsics, w2c, draws, kf_w2c, *, valid_idx=None, n_valid_idx=None, kf_masks=None, edge=20,
                     want_valid=True, want_pts=False):
    """fr_keyframe_overlap: dict(counts int32 [K], status int32 [4] = {valid points, out-of-range draws, 0, 0}, valid uint8 [n] or
    None, pts float32 [n,3] or None), all on the device of `depth`.  draws: int64 [n] (host or device) into valid_idx -- the list
    `keyframe_valid_pixels` wrote, with n_valid_idx its count as the host read it -- or, without valid_idx, flat pixel indices.
    kf_w2c: [K,4,4] float32 on the device (K may be 0).  kf_masks: None, or one entry per keyframe, each None or a [H,W] mask on the
    device (bool / uint8; anything else is compared with 0).  intrinsics [3,3] and w2c [4,4] may live anywhere.  No host read and no
    host synchronisation in here; the number of launches does not depend on K."""
    H, W = _depth_hw(depth)
    dev = depth.device
    d = _host_i64_to(draws, dev).reshape(-1)
    n = int(d.numel())
    kf = kf_w2c if isinstance(kf_w2c, torch.Tensor) else torch.as_tensor(kf_w2c, dtype=torch.float32)
    K = int(kf.shape[0]) if kf.dim() == 3 else (0 if kf.numel() == 0 else -1)
    if K < 0 or (K > 0 and tuple(kf.shape[1:]) != (4, 4)):
        raise FisherRastError(f"keyframe overlap: kf_w2c must be [K,4,4], got {tuple(kf.shape)}")
    kf = _prep(kf, dev)
    Kmat, pose = _small_f32(intrinsics, dev, 3, 3, "intrinsics"), _small_f32(w2c, dev, 4, 4, "w2c")
    if valid_idx is not None:
        if valid_idx.device != dev or valid_idx.dtype != torch.int32 or not valid_idx.is_contiguous():
            raise FisherRastError("keyframe overlap: valid_idx must be a contiguous int32 tensor on the device of depth")
        n_valid_idx = int(valid_idx.numel() if n_valid_idx is None else n_valid_idx)
        if not 0 <= n_valid_idx <= valid_idx.numel():
            raise FisherRastError(f"keyframe overlap: n_valid_idx {n_valid_idx} outside valid_idx of {valid_idx.numel()}")
    keep, table = [], None
    if kf_masks is not None and any(m is not None for m in kf_masks):
        if len(kf_masks) != K:
            raise FisherRastError(f"keyframe overlap: {len(kf_masks)} masks for {K} keyframes")
        keep = [None if m is None else _mask_bytes_hw(m if m.device == dev else m.to(dev), H, W, "keyframe mask") for m in kf_masks]
        table = _host_i64_to([0 if m is None else m.data_ptr() for m in keep], dev)
    lib = _lib.load()
    ws = _keyframe_workspace("overlap", (n,), dev, int(lib.fr_keyframe_overlap_workspace_bytes(n)))
    counts = torch.empty((K,), dtype=torch.int32, device=dev)
    status = torch.empty((_lib.FR_KEYFRAME_STATUS_WORDS,), dtype=torch.int32, device=dev)
    valid = torch.empty((n,), dtype=torch.uint8, device=dev) if want_valid else None
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev) if want_pts else None
    cfg = KeyframeCfg(H, W, n, K, int(edge), int(n_valid_idx or 0), Kmat.data_ptr(), pose.data_ptr())
    with torch.cuda.device(dev):
        _lib.check(lib.fr_keyframe_overlap(ctypes.byref(cfg), _ptr(depth), _ptr(valid_idx), _ptr(d), _ptr(kf), _ptr(table),
                                           _ptr(counts) if K else None, _ptr(valid), _ptr(pts), _ptr(status), _ptr(ws),
                                           ws.numel() * ws.element_size(), _stream(dev)), "fr_keyframe_overlap")
    del keep                                                   # alive until the launches were issued; the stream orders the rest
    return dict(counts=counts, status=status, valid=valid, pts=pts)


# ---- fused render-variable build (fr_rendervar_forward / fr_rendervar_backward) -------------------------------------------------------

class RenderVarUnsupported(FisherRastError):
    """the inputs are outside what the render-variable kernels take (not float32, not contiguous, not on one HIP device, log_scales not
    1 or 3 wide): raised before anything is launched, so a caller may take the torch route for this call instead"""


RENDERVAR_INPUTS = ("cam_unnorm_rots", "cam_trans", "first_frame_w2c", "means3D", "unnorm_rotations", "logit_opacities", "log_scales")
_RENDERVAR_COLS = {"means3D": 3, "unnorm_rotations": 4, "logit_opacities": 1}


def rendervar_check(tensors, time_idx, need_cuda=True):
    """(P, scale_cols, n_frames) of the inputs in `tensors` (name -> tensor or None), or RenderVarUnsupported"""
    present = {k: v for k, v in tensors.items() if v is not None}
    dev = None
    for k, v in present.items():
        if v.dtype != torch.float32 or not v.is_contiguous():
            raise RenderVarUnsupported(f"rendervar: {k} must be contiguous float32 (got {v.dtype}, contiguous={v.is_contiguous()})")
        if need_cuda and not v.is_cuda:
            raise RenderVarUnsupported(f"rendervar: {k} must live on a HIP device")
        if dev is not None and v.device != dev:
            raise RenderVarUnsupported(f"rendervar: {k} is on {v.device}, other inputs on {dev}")
        dev = v.device
    rows = {int(v.shape[0]) for k, v in present.items() if k in _RENDERVAR_COLS or k == "log_scales"}
    for k, cols in _RENDERVAR_COLS.items():
        if k in present and (present[k].dim() != 2 or int(present[k].shape[1]) != cols):
            raise RenderVarUnsupported(f"rendervar: {k} must be [P,{cols}] (got {tuple(present[k].shape)})")
    scale_cols = 3
    if "log_scales" in present:
        ls = present["log_scales"]
        if ls.dim() != 2 or int(ls.shape[1]) not in (1, 3):
            raise RenderVarUnsupported(f"rendervar: log_scales must be [P,1] or [P,3] (got {tuple(ls.shape)})")
        scale_cols = int(ls.shape[1])
    if len(rows) > 1:
        raise RenderVarUnsupported(f"rendervar: the per-Gaussian inputs disagree on P ({sorted(rows)})")
    n_frames = 1
    if "cam_unnorm_rots" in present or "cam_trans" in present:
        cr, ct = present.get("cam_unnorm_rots"), present.get("cam_trans")
        if cr is None or ct is None or cr.dim() != 3 or ct.dim() != 3 or tuple(cr.shape[:2]) != (1, 4) or tuple(ct.shape[:2]) != (1, 3) or cr.shape[2] != ct.shape[2]:
            raise RenderVarUnsupported("rendervar: the camera arrays must be [1,4,T] and [1,3,T]")
        n_frames = int(cr.shape[2])
        if not 0 <= int(time_idx) < n_frames:
            raise RenderVarUnsupported(f"rendervar: time_idx {time_idx} is outside [0, {n_frames})")
    if "first_frame_w2c" in present and tuple(present["first_frame_w2c"].shape) != (4, 4):
        raise RenderVarUnsupported("rendervar: first_frame_w2c must be [4,4]")
    return (rows.pop() if rows else 0), scale_cols, n_frames


def rendervar_cfg(P, scale_cols, time_idx, n_frames, tensors):
    """fr_rendervar_cfg over `tensors` (field name -> tensor or None; a missing field is a null pointer)"""
    cfg = _lib.RenderVarCfg(int(P), int(scale_cols), int(time_idx), int(n_frames))
    for name, t in tensors.items():
        setattr(cfg, name, None if t is None else t.data_ptr())
    return cfg


def rendervar_forward(P, scale_cols, time_idx, n_frames, tensors):
    """one fr_rendervar_forward call on the current stream of the tensors' device"""
    dev = next(t for t in tensors.values() if t is not None).device
    cfg = rendervar_cfg(P, scale_cols, time_idx, n_frames, tensors)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_rendervar_forward(ctypes.byref(cfg), _stream(dev)), "fr_rendervar_forward")


_rendervar_ws = {}


def rendervar_backward(P, scale_cols, time_idx, n_frames, tensors):
    """one fr_rendervar_backward call; the camera sums' workspace is kept per (device, stream) and only ever grown"""
    dev = next(t for t in tensors.values() if t is not None).device
    lib = _lib.load()
    cfg = rendervar_cfg(P, scale_cols, time_idx, n_frames, tensors)
    ws, nbytes = None, 0
    if tensors.get("g_cam_unnorm_rots") is not None or tensors.get("g_cam_trans") is not None:
        nbytes = int(lib.fr_rendervar_workspace_bytes(int(P)))
        key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(dev).cuda_stream))
        ws = _rendervar_ws.get(key)
        if ws is None or ws.numel() * 4 < nbytes:
            ws = _rendervar_ws[key] = torch.empty((max(nbytes // 4, 12 * 2048),), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(lib.fr_rendervar_backward(ctypes.byref(cfg), None if ws is None else ws.data_ptr(), 0 if ws is None else ws.numel() * 4, _stream(dev)),
                   "fr_rendervar_backward")


# ---- render-quality evaluation (fr_view_metrics) --------------------------------------------------------------------------------

_view_metrics_ws = {}


def _view_metrics_workspace(dev, nbytes):
    """the partial sums' workspace, kept per (device, stream) and only ever grown, as `_backward_scratch` is"""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), int(torch.cuda.current_stream(dev).cuda_stream))
    ws = _view_metrics_ws.get(key)
    if ws is None or ws.numel() * 8 < nbytes:
        _view_metrics_ws[key] = None
        ws = _view_metrics_ws[key] = torch.empty((nbytes // 8 + (nbytes >> 5),), dtype=torch.float64, device=dev)
    return ws


def _view_images(t, name, V, H, W, dev):
    """(tensor, view stride in elements) of a float32 [V,1,H,W] or [V,H,W] whose H W blocks are contiguous; the views may be strided
    (channel 0 of a [V,3,H,W] tensor is taken where it lies, not copied)"""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dev:
        raise ValueError(f"view_metrics: {name} must be a float32 tensor on {dev}")
    if t.dim() == 4 and t.shape[1] == 1:
        t = t[:, 0]
    if tuple(t.shape) != (V, H, W):
        raise ValueError(f"view_metrics: {name} of shape {tuple(t.shape)} does not fit [{V},1,{H},{W}] or [{V},{H},{W}]")
    inner = (W == 1 or t.stride(2) == 1) and (H == 1 or t.stride(1) == W)
    if not inner or (V > 1 and t.stride(0) < H * W):
        raise ValueError(f"view_metrics: the H W block of every view of {name} must be contiguous (strides {tuple(t.stride())})")
    return t, (int(t.stride(0)) if V > 1 else H * W)


def view_metrics(render, gt_rgb, depth=None, gt_depth=None, mask=None, clamp=True, depth_valid_only=False, out=None):
    """PSNR, SSIM and depth error of V rendered views against their ground truth in one call (fr_view_metrics, include/fisher_rast.h):
    {"rows": [V,8] = {psnr, ssim, depth_l1, depth_rmse, mse_r, mse_g, mse_b, depth_count} per view, "summary": [8] = {views kept,
    mean psnr, mean ssim, mean depth_l1, mean depth_rmse, 0, 0, V}} on the device, on torch's current stream, without a synchronisation.
    render: float32 [V,3,H,W]; gt_rgb: float32 [V,3,H,W] or uint8 [V,H,W,3|4] (value / 255, channels 0..2); depth / gt_depth: float32
    [V,1,H,W] or [V,H,W], both or neither, the views may be strided; mask: bool / uint8 [V,H,W] or [V,1,H,W].  `clamp`: the render is
    clamped to [0,1] first (eval_navigation); `depth_valid_only`: the depth terms over the pixels with gt_depth > 0 (report_progress).
    `out`: a dict that may hold contiguous float32 device tensors "rows" [V,8] and "summary" [8], written instead of fresh ones.
    Anything else -- another dtype or device, an H W block that is not contiguous -- raises ValueError."""
    if not isinstance(render, torch.Tensor) or not render.is_cuda or render.dtype != torch.float32 or render.dim() != 4 or render.shape[1] != 3:
        raise ValueError("view_metrics: render must be a float32 [V,3,H,W] tensor on a HIP device")
    dev = render.device
    V, _, H, W = (int(s) for s in render.shape)
    if V < 1 or H < 1 or W < 1:
        raise ValueError(f"view_metrics: an empty render {tuple(render.shape)}")
    inner = render[0].is_contiguous() and (V == 1 or render.stride(0) >= 3 * H * W)
    if not inner:
        raise ValueError(f"view_metrics: the [3,H,W] block of every view of render must be contiguous (strides {tuple(render.stride())})")
    if not isinstance(gt_rgb, torch.Tensor) or gt_rgb.device != dev or not gt_rgb.is_contiguous():
        raise ValueError(f"view_metrics: gt_rgb must be a contiguous tensor on {dev}")
    if gt_rgb.dtype == torch.float32 and tuple(gt_rgb.shape) == (V, 3, H, W):
        layout, channels = _lib.FR_EVAL_GT_F32_CHW, 3
    elif gt_rgb.dtype == torch.uint8 and gt_rgb.dim() == 4 and tuple(gt_rgb.shape[:3]) == (V, H, W) and gt_rgb.shape[3] in (3, 4):
        layout, channels = _lib.FR_EVAL_GT_U8_HWC, int(gt_rgb.shape[3])
    else:
        raise ValueError(f"view_metrics: gt_rgb must be float32 [{V},3,{H},{W}] or uint8 [{V},{H},{W},3|4], not {gt_rgb.dtype} {tuple(gt_rgb.shape)}")
    if (depth is None) != (gt_depth is None):
        raise ValueError("view_metrics: depth and gt_depth go together (both or neither)")
    dvs = gvs = H * W
    if depth is not None:
        depth, dvs = _view_images(depth, "depth", V, H, W, dev)
        gt_depth, gvs = _view_images(gt_depth, "gt_depth", V, H, W, dev)
    m = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != dev or mask.dtype not in (torch.bool, torch.uint8) or mask.numel() != V * H * W:
            raise ValueError(f"view_metrics: mask must be a bool or uint8 [{V},{H},{W}] tensor on {dev}")
        m = mask.reshape(V, H, W).contiguous()
        m = m.view(torch.uint8) if m.dtype == torch.bool else m
    given = out or {}

    def new(name, *shape):
        t = given.get(name)
        if t is None:
            return torch.empty(shape, dtype=torch.float32, device=dev)
        if tuple(t.shape) != shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"view_metrics: out['{name}'] must be a contiguous float32 tensor of shape {shape} on {dev}")
        return t
    rows, summary = new("rows", V, _lib.FR_EVAL_ROW), new("summary", _lib.FR_EVAL_ROW)
    lib = _lib.load()
    nbytes = int(lib.fr_view_metrics_workspace_bytes(V, H, W))
    if nbytes == 0:
        raise ValueError(f"view_metrics: {V} views of {H} x {W} are outside the library's limits (V <= 65535, H W <= 2^30)")
    cfg = _lib.ViewMetricsCfg(V, H, W, layout, channels, int(bool(clamp)), int(bool(depth_valid_only)),
                              int(render.stride(0)) if V > 1 else 3 * H * W, dvs, gvs)
    with torch.cuda.device(dev):
        ws = _view_metrics_workspace(dev, nbytes)
        _lib.check(lib.fr_view_metrics(ctypes.byref(cfg), render.data_ptr(), None if depth is None else depth.data_ptr(), gt_rgb.data_ptr(),
                                       None if gt_depth is None else gt_depth.data_ptr(), None if m is None else m.data_ptr(),
                                       rows.data_ptr(), summary.data_ptr(), ws.data_ptr(), ws.numel() * 8, _stream(dev)), "fr_view_metrics")
    return {"rows": rows, "summary": summary}


def view_metrics_summary(rows, out=None):
    """The summary [8] over rows [V,8] that several `view_metrics` calls filled slice by slice: one launch on the current stream."""
    if not isinstance(rows, torch.Tensor) or not rows.is_cuda or rows.dtype != torch.float32 or rows.dim() != 2 \
            or rows.shape[1] != _lib.FR_EVAL_ROW or rows.shape[0] < 1 or not rows.is_contiguous():
        raise ValueError("view_metrics_summary: rows must be a contiguous float32 [V,8] tensor on a HIP device, V >= 1")
    dev = rows.device
    summary = torch.empty((_lib.FR_EVAL_ROW,), dtype=torch.float32, device=dev) if out is None else out
    with torch.cuda.device(dev):
        _lib.check(_lib.load().fr_view_metrics_summary(rows.data_ptr(), int(rows.shape[0]), summary.data_ptr(), _stream(dev)),
                   "fr_view_metrics_summary")
    return summary
