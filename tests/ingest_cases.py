"""Inputs, a binary32 NumPy restatement and the reference-order torch chain for the frame ingest (fr_frame_ingest_select / _emit).

The cases are regenerated from seeds, not stored.  `np_select` / `np_emit` restate csrc/fr_ingest_math.h in NumPy binary32 with the
header's operand order: every operation is one of + - x / sqrt, each correctly rounded in both, so they reproduce the header bit
for bit -- all but logf.  `torch_non_presence` / `torch_pointcloud` are the reference's chain (models/SLAM/gaussian.py:320-342,
75-143: torch.median, max_pool2d, torch.inverse, matmul, boolean indexing) in this helper's own form, on any device and dtype.
The g++ harness over the header (tests/harness/fr_ingest_harness.cpp) is bound here too."""

import numpy as np

import cameras
import harness_build

FAMILIES = ["half", "all", "none", "ties", "prefix-hi", "prefix-lo", "nan", "inf", "last-pixel", "pool-corner"]
# (H, W, d): one pixel; odd n; a 2 x 2 pool; one workgroup exactly at three poolings; ragged workgroups; pooled 12 x 16; and several
# workgroups in the scan of the counts (256 workgroups at d = 1, 16 at d = 4) -- these two with one family each
SMALL_SHAPES = [(1, 1, 1), (5, 7, 1), (4, 6, 2), (16, 16, 1), (16, 16, 2), (16, 16, 4), (37, 53, 1), (48, 64, 4)]
LARGE_CASES = [("half", (256, 256, 1)), ("pool-corner", (256, 256, 4))]
ALL_CASES = [(f, s) for s in SMALL_SHAPES for f in FAMILIES] + LARGE_CASES
SIL_THRES = 0.5
NAN_BITS = 0x7FC00000
# world points: |got - binary64 chain| <= K 2^-24 sum_j |c2w_ij| |p_j|.  Needed on the CPU over every case and both cameras below: 4.49
# (printed by tests/test_frame_ingest_cpu.py, which fails when the measurement moves away from the figure recorded here and in
# DESIGN.md section 2); K used is twice that, under the cap of 16.
K_NEEDED_CPU = 4.49
K_POINTS = min(16.0, round(2 * K_NEEDED_CPU, 1))


def case_id(c):
    return f"{c[0]}-{c[1][0]}x{c[1][1]}d{c[1][2]}"


def camera(H, W, which=0):
    """(K [3,3], w2c [4,4]) float32: the off-centre anisotropic camera of tests/cameras.py at this size, under one of its
    rotation + translation poses"""
    cw, ch, K = cameras.CAMERAS["offcentre"]
    sx, sy = W / cw, H / ch
    K = np.array([[K[0][0] * sx, 0, K[0][2] * sx], [0, K[1][1] * sy, K[1][2] * sy], [0, 0, 1]], np.float32)
    w2c = cameras.pose() if which == 0 else cameras.small_rotation()
    return K, np.ascontiguousarray(w2c, np.float32)


def make_case(family, shape, which_camera=0):
    """dict(depth_sil [3,H,W], gt [1,H,W], color [3,H,W], K, w2c, ratio, H, W, d), float32"""
    H, W, d = shape
    rng = np.random.default_rng([H, W, d, FAMILIES.index(family), 20250301])
    n = H * W
    gt = rng.uniform(0.5, 4.0, (H, W)).astype(np.float32)
    gt[rng.uniform(size=(H, W)) < 0.05] = 0.0                                   # unmeasured pixels
    gt[rng.uniform(size=(H, W)) < 0.03] = np.float32(0.005)                     # measured, but under the 0.01 cut
    render = (gt + rng.normal(0, 0.2, (H, W)) * (rng.uniform(size=(H, W)) < 0.7)).astype(np.float32)
    sil = np.ones((H, W), np.float32)
    ratio = 2.0
    if family == "half":
        sil[:, :W // 2] = 0.0
    elif family == "all":
        sil[:] = 0.0
        gt = np.maximum(gt, np.float32(0.02))
    elif family == "none":
        gt[:] = 0.0
        sil[:] = 0.0
    elif family == "ties":                                                      # every error is 0.5: one bucket in every round
        gt[:] = 2.0
        render[:] = 2.5
        sil[rng.uniform(size=(H, W)) < 0.2] = 0.0
        ratio = 1.0                                                             # thr == err: "greater" must stay false everywhere
    elif family in ("prefix-hi", "prefix-lo"):
        # err == gt exactly (render = 2 gt): bit patterns that differ in the top byte only / in the lowest byte only
        if family == "prefix-hi":
            bits = (rng.integers(0x38, 0x48, n, dtype=np.uint32) << np.uint32(24)) | np.uint32(0x2ABCDE)
        else:
            bits = np.uint32(0x3FC5A300) | rng.integers(0, 256, n, dtype=np.uint32)
        gt = bits.view(np.float32).reshape(H, W).copy()
        render = (gt * np.float32(2.0)).astype(np.float32)
        ratio = 1.0                                                             # selected: the errors above the median
    elif family == "nan":
        sil[:, :W // 2] = 0.0
        gt.reshape(-1)[n // 3] = 1.5
        render.reshape(-1)[n // 3] = np.nan
    elif family == "inf":
        sil[:, :W // 2] = 0.0
        gt.reshape(-1)[[n // 3, n - 1]] = 1.5
        render.reshape(-1)[[n // 3, n - 1]] = np.inf                           # err = inf, and render > gt
    elif family == "last-pixel":
        render = gt.copy()
        gt[-1, -1] = 1.25
        sil[-1, -1] = 0.0
    elif family == "pool-corner":
        render = gt.copy()
        gt[d - 1::d, d - 1::d] = np.float32(1.75)
        sil[d - 1::d, d - 1::d] = 0.0
        if d > 1:
            gt[::d, ::d] = 0.0                                                  # the sampled pixel of every block has no depth
    else:
        raise ValueError(family)
    depth_sil = np.stack([render, sil, render * render]).astype(np.float32)
    color = rng.uniform(0, 1, (3, H, W)).astype(np.float32)
    K, w2c = camera(H, W, which_camera)
    return dict(depth_sil=depth_sil, gt=gt[None].copy(), color=color, K=K, w2c=w2c, ratio=float(ratio), H=H, W=W, d=d, family=family)


# ---- the binary32 restatement of csrc/fr_ingest_math.h ---------------------------------------------------------------------------

F = np.float32


def np_depth_error(gt, render):
    with np.errstate(invalid="ignore"):
        return (np.abs(gt - render) * (gt > 0).astype(F)).astype(F)


def np_median_bits(err):
    """(bits of element (n - 1) // 2 of the sorted values, or NAN_BITS; has_nan)"""
    e = err.reshape(-1)
    if np.isnan(e).any():
        return NAN_BITS, 1
    return int(np.sort(e.view(np.uint32))[(e.size - 1) // 2]), 0


def np_pool(mask, d):
    H, W = mask.shape
    return mask.reshape(H // d, d, W // d, d).any(axis=(1, 3))


def np_select(c, mask_in=None, obj_mask=None):
    """dict(pixel_mask [H,W] bool, pooled [G] bool, idx int32, count, median_bits, has_nan) -- the predicate when mask_in is None,
    ANDed with obj_mask [H,W] where given"""
    med, has_nan = 0, 0
    if mask_in is None:
        render, sil, gt = c["depth_sil"][0], c["depth_sil"][1], c["gt"][0]
        err = np_depth_error(gt, render)
        med, has_nan = np_median_bits(err)
        with np.errstate(invalid="ignore"):
            thr = F(c["ratio"]) * np.array([med], np.uint32).view(F)[0]
            pm = (sil < F(SIL_THRES)) | ((render > gt) & (err > thr))
        if obj_mask is not None:
            pm &= np.asarray(obj_mask).reshape(c["H"], c["W"]) != 0
        pm &= gt > F(0.01)
    else:
        pm = np.asarray(mask_in).reshape(c["H"], c["W"]) != 0
    pooled = np_pool(pm, c["d"]).reshape(-1)
    idx = np.flatnonzero(pooled).astype(np.int32)
    return dict(pixel_mask=pm, pooled=pooled, idx=idx, count=int(idx.size), median_bits=med, has_nan=has_nan)


def np_invert_affine(w2c):
    a = np.asarray(w2c, F)
    t = a[:3, 3]
    c = np.empty((3, 3), F)
    c[0, 0] = a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1]; c[0, 1] = a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2]; c[0, 2] = a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]
    c[1, 0] = a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2]; c[1, 1] = a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0]; c[1, 2] = a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]
    c[2, 0] = a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0]; c[2, 1] = a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1]; c[2, 2] = a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]
    det = (a[0, 0] * c[0, 0] + a[0, 1] * c[1, 0]) + a[0, 2] * c[2, 0]
    inv = (c / det).astype(F)
    m = np.empty((3, 4), F)
    m[:, :3] = inv
    m[:, 3] = -((inv[:, 0] * t[0] + inv[:, 1] * t[1]) + inv[:, 2] * t[2])
    return m


def np_emit(c, idx=None, transform_pts=True, scale_cols=3):
    """dict(means [N,3], rgb [N,3], msd [N], log_scales64 [N] (binary64 of the binary32 msd), rot, opac) for the cells idx (None: all)"""
    H, W, d = c["H"], c["W"], c["d"]
    Gw = W // d
    g = np.arange((H // d) * Gw) if idx is None else np.asarray(idx, np.int64)
    x, y = (g % Gw) * d, (g // Gw) * d
    K = c["K"]
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    z = c["gt"][0][y, x]
    xx, yy = (x.astype(F) - cx) / fx, (y.astype(F) - cy) / fy
    X, Y = xx * z, yy * z
    if transform_pts:
        m = np_invert_affine(c["w2c"])
        means = np.stack([((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1).astype(F)
    else:
        means = np.stack([X, Y, z], 1).astype(F)
    s = (F(d) * z) / ((fx + fy) / F(2.0))
    msd = (s * s).astype(F)
    with np.errstate(divide="ignore"):
        log64 = np.log(np.sqrt(msd).astype(np.float64))          # sqrt in binary32 (exact rounding), log in binary64
    n = g.size
    rot = np.zeros((n, 4), F); rot[:, 0] = 1.0
    return dict(means=means, rgb=np.ascontiguousarray(c["color"][:, y, x].T), msd=msd, log_scales64=log64, rot=rot, opac=np.zeros((n, 1), F))


def log_scale_ok(got, want64):
    """within 2 ulp32(|v|) + 2^-23 of the binary64 value: sqrtf is exact, logf is good to 1 ulp, and the 2^-24 relative error of its
    binary32 argument moves the log by 6e-8 absolutely; infinities (a depth of 0 or an overflow) must agree exactly"""
    got, want64 = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    fin = np.isfinite(want64)
    ok = np.array_equal(got[~fin], want64[~fin])
    tol = 2.0 * np.spacing(np.abs(want64[fin]).astype(F)).astype(np.float64) + 2.0 ** -23
    return bool(ok and (np.abs(got[fin] - want64[fin]) <= tol).all())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- the reference-order chain in torch ------------------------------------------------------------------------------------------

def torch_non_presence(depth_sil, gt_depth, sil_thres, ratio, obj_mask_2d=None):
    """(flat bool mask [H W], median 0-dim) as gaussian.py:329-342 forms them -- with `obj_mask_2d` [H,W] as gaussian_object.py:440-463
    do, which AND it in before the depth filter; tensors on any device"""
    import torch
    sil, render, gt = depth_sil[1], depth_sil[0], gt_depth[0]
    err = torch.abs(gt - render) * (gt > 0)
    med = err.median()
    by_depth = (render > gt) * (err > ratio * med)
    mask = (sil < sil_thres) | by_depth
    if obj_mask_2d is not None:
        mask = mask & obj_mask_2d.bool()
    mask = mask.reshape(-1) & (gt > 0.01).reshape(-1)
    return mask, med


def torch_pointcloud(color, depth, K, w2c, transform_pts=True, downsample=1, mask=None, dtype=None):
    """(point_cld [N,6], mean3_sq_dist [N], c2w [4,4], pts_cam4 [N,4]) as gaussian.py:83-136 forms them, in `dtype` (default: the
    inputs'); an all-zero mask keeps every point, as there"""
    import torch
    import torch.nn.functional as Fn
    dtype = dtype or depth.dtype
    dev = depth.device
    color, depth, K, w2c = color.to(dtype), depth.to(dtype), K.to(dtype), w2c.to(dtype)
    H, W = color.shape[1], color.shape[2]
    xg, yg = torch.meshgrid(torch.arange(0, W, downsample, device=dev).to(dtype), torch.arange(0, H, downsample, device=dev).to(dtype), indexing="xy")
    xx, yy = ((xg - K[0][2]) / K[0][0]).reshape(-1), ((yg - K[1][2]) / K[1][1]).reshape(-1)
    z = depth[0, ::downsample, ::downsample].reshape(-1)
    cam4 = torch.stack((xx * z, yy * z, z, torch.ones_like(z)), dim=-1)
    c2w = torch.inverse(w2c) if transform_pts else torch.eye(4, dtype=dtype, device=dev)
    pts = (c2w @ cam4.T).T[:, :3] if transform_pts else cam4[:, :3]
    msd = (downsample * z / ((K[0][0] + K[1][1]) / 2)) ** 2
    cols = color[:, ::downsample, ::downsample].permute(1, 2, 0).reshape(-1, 3)
    cld = torch.cat((pts, cols), -1)
    if mask is not None:
        keep = Fn.max_pool2d(mask.reshape(1, H, W).float(), downsample).bool().reshape(-1)
        if keep.sum() > 0:
            cld, msd, cam4 = cld[keep], msd[keep], cam4[keep]
    return cld, msd, c2w, cam4


def points_need(got, c, idx, transform_pts=True):
    """max over the rows of |got - binary64 chain| / (2^-24 sum_j |c2w_ij| |p_j|): the K that the rule would have to hold"""
    import torch
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    cld, _, c2w, cam4 = torch_pointcloud(t(c["color"]), t(c["gt"]), t(c["K"]), t(c["w2c"]), transform_pts, c["d"], None, torch.float64)
    sel = slice(None) if idx is None else np.asarray(idx, np.int64)
    want, cam4, c2w = cld.numpy()[sel, :3], np.abs(cam4.numpy()[sel]), np.abs(c2w.numpy()[:3])
    scale = 2.0 ** -24 * cam4 @ c2w.T
    dev = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        need = np.where(dev == 0, 0.0, dev / scale)
    return float(need.max()) if need.size else 0.0


# ---- the g++ harness over csrc/fr_ingest_math.h (tests/harness/fr_ingest_harness.cpp) --------------------------------------------

def build_harness():
    import ctypes
    h = ctypes.CDLL(harness_build.shared("fr_ingest_harness"))
    vp = ctypes.c_void_p
    h.fri_select.argtypes = [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [vp] * 7
    h.fri_select.restype = None
    h.fri_inverse.argtypes = [vp, vp]
    h.fri_inverse.restype = None
    h.fri_emit.argtypes = [ctypes.c_int] * 5 + [vp] * 5 + [ctypes.c_int, ctypes.c_longlong] + [vp] * 6
    h.fri_emit.restype = None
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def harness_select(h, c, mask_in=None, obj_mask=None):
    """mask_in: the mask itself (mode 1); obj_mask: ANDed into the predicate (mode 0)"""
    H, W, d = c["H"], c["W"], c["d"]
    G = (H // d) * (W // d)
    pm, pooled, idx, status = np.zeros(H * W, np.uint8), np.zeros(G, np.uint8), np.zeros(G, np.int32), np.zeros(5, np.int32)
    given = mask_in if mask_in is not None else obj_mask
    m = None if given is None else np.ascontiguousarray(given, np.uint8)
    h.fri_select(H, W, d, 0 if mask_in is None else 1, SIL_THRES, c["ratio"], _ptr(c["depth_sil"]), _ptr(c["gt"]), _ptr(m),
                 _ptr(pm), _ptr(pooled), _ptr(idx), _ptr(status))
    n = int(status[0])
    return dict(pixel_mask=pm.reshape(H, W).astype(bool), pooled=pooled.astype(bool), idx=idx[:n].copy(), count=n,
                median_bits=int(np.uint32(status[4])), has_nan=int(status[1]))


def harness_emit(h, c, idx=None, transform_pts=True, scale_cols=3, row_offset=0):
    H, W, d = c["H"], c["W"], c["d"]
    n = (H // d) * (W // d) if idx is None else len(idx)
    rows = row_offset + n
    out = dict(means=np.zeros((rows, 3), F), rgb=np.zeros((rows, 3), F), rot=np.zeros((rows, 4), F), opac=np.ones((rows, 1), F),
               log_scales=np.zeros((rows, scale_cols), F), msd=np.zeros(rows, F))
    ix = None if idx is None else np.ascontiguousarray(idx, np.int32)
    h.fri_emit(H, W, d, int(transform_pts), scale_cols, _ptr(c["K"]), _ptr(c["w2c"]), _ptr(c["color"]), _ptr(c["gt"]), _ptr(ix), n, row_offset,
               *(_ptr(out[k]) for k in ("means", "rgb", "rot", "opac", "log_scales", "msd")))
    return out
