"""Inputs, restatements and the g++ harness for the object-aware training step (fr_loss_mask, fr_bg_penalty_forward / _backward,
fr_outside_mask; csrc/fr_objloss.hip over csrc/fr_objloss_math.h).

The cases are regenerated from seeds, not stored.  Mask families (`make_mask_case`): every predicate of the rule about half true;
a NaN in the rendered depth; +inf depth with +inf depth^2 (the variance proxy is NaN, and at an unmeasured pixel the error is too); a
frame without a measured depth (median 0: nothing passes the strict `<`); more than half unmeasured (median 0 through ties); a plateau
of equal errors across the median position; an error exactly equal to 10 x the median; a silhouette exactly equal to the threshold;
-0.0 among the measured depths.  Penalty families (`make_penalty_case`): negative values, exact zeros, a NaN inside and outside the
object, silhouettes at -0.5, 0, 1, 1.5, NaN and +inf.  Outside-mask families (`make_outside_case`): an exact one (axis-permutation
rotation, integer translation, means on multiples of 2^-6, power-of-two focal lengths, integer principal points: every sum is exact
in any order) and a general camera."""
import ctypes
import os

import numpy as np
import harness_build

F = np.float32
SHAPES = [(1, 1), (1, 7), (5, 7), (16, 16), (37, 53), (64, 65)]          # n odd and even, one pixel, more than one workgroup
GPU_SHAPE = (256, 256)                                                    # once, on the GPU
MASK_FAMILIES = ["half", "nan_depth", "inf_depth", "gt_zero", "mostly_unmeasured", "plateau", "ten_med", "sil_at_thres", "neg_zero_gt"]
OBJ_KINDS = ["none", "ones", "zeros", "half"]                             # as bytes; OBJ_FORMS are the layouts the Python layer takes
OBJ_FORMS = ["bool", "uint8", "float", "hw1"]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]      # (reject_outliers, need_presence)
PENALTY_FAMILIES = ["plain", "zeros", "nan_inside", "nan_outside", "sil_edges", "sil_nan", "sil_inf"]
PENALTY_OBJ = ["ones", "zeros", "half"]                                   # n = 0 (denominators 1), all background, half
SIL_THRES = 0.89                                                          # float32(0.89) > 0.89 is false: the comparison must be binary32
RATIO = 10.0
LAMBDA = 0.1
UPSTREAM = 0.37                                                           # not 1: the backward has to read it

OUTSIDE_P = [1, 63, 64, 65, 4096]
OUTSIDE_MASKS = [(37, 53), (48, 64)]
NAN_BITS = 0x7fc00000


def _rng(*key):
    return np.random.default_rng([int(k) for k in key] + [20250517])


def make_obj(shape, kind, seed=0):
    """the object mask as bytes [H,W], or None"""
    H, W = shape
    if kind == "none":
        return None
    if kind == "ones":
        return np.ones((H, W), np.uint8)
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    return (_rng(H, W, 7, seed).uniform(size=(H, W)) < 0.5).astype(np.uint8)


def obj_form(obj, form):
    """the bytes in one of the layouts a caller may hand over (a torch tensor)"""
    import torch
    t = torch.from_numpy(obj)
    if form == "bool":
        return t.bool()
    if form == "uint8":
        return t * 3                                                       # any non-zero byte is object
    if form == "float":
        return t.float() * 0.5
    return t.bool().unsqueeze(-1)                                          # [H,W,1]


def make_mask_case(shape, family):
    """(depth_sil [3,H,W], gt [1,H,W]) float32"""
    H, W = shape
    n = H * W
    rng = _rng(H, W, MASK_FAMILIES.index(family))
    gt = rng.integers(4, 40, n).astype(F) * F(0.25)                        # multiples of 1/4 in [1, 10)
    measured = rng.uniform(size=n) < 0.6
    err = (F(10.0) ** rng.uniform(-2, 2, n)).astype(F) * F(0.05)          # four decades: ten times the median cuts them about in half
    sil = rng.uniform(0.78, 1.0, n).astype(F)
    var_nan = rng.uniform(size=n) < 0.5 if family == "half" else np.zeros(n, bool)
    if family == "gt_zero":
        measured[:] = False
    elif family == "mostly_unmeasured":
        measured = rng.uniform(size=n) < 0.3
    elif family == "plateau":
        err = rng.choice(np.array([0.125, 0.5, 0.5, 0.5, 2.0, 8.0], F), n)        # gt - err is exact: equal errors straddle the median
        measured[:] = True
    elif family == "ten_med":
        err = rng.choice(np.array([0.125, 0.125, 0.125, 0.125, 1.25, 1.0, 2.0], F), n)
        measured[:] = True
        err[: min(n, 3)] = np.array([0.125, 1.25, 0.125], F)[: min(n, 3)]  # (n = 1: the error is the median)
    elif family == "sil_at_thres":
        t = F(SIL_THRES)
        sil = rng.choice(np.array([t, np.nextafter(t, F(2)), np.nextafter(t, F(0)), F(0.95), F(0.5)], F), n)
    gt = np.where(measured, gt, F(0.0)).astype(F)
    if family == "neg_zero_gt":
        gt[(gt == 0) & (rng.uniform(size=n) < 0.5)] = F(-0.0)              # half of the unmeasured pixels
    d = (gt - err * rng.choice(np.array([-1.0, 1.0], F), n)).astype(F)
    d = np.where(gt > 0, d, rng.uniform(0.5, 9.0, n).astype(F)).astype(F)   # the map renders something where nothing was measured
    d2 = (d * d + F(0.01)).astype(F)
    d2[var_nan] = np.nan
    if family == "nan_depth":
        d[rng.integers(0, n, max(1, n // 50))] = np.nan
    elif family == "inf_depth":
        hit = rng.integers(0, n, max(1, n // 50))
        d[hit] = np.inf
        d2[hit] = np.inf
        gt[hit[0]] = F(0.0)                                                # at least one of them unmeasured: |0 - inf| * 0 is NaN
    ds = np.stack([d, sil, d2]).reshape(3, H, W).astype(F)
    return np.ascontiguousarray(ds), np.ascontiguousarray(gt.reshape(1, H, W))


def make_penalty_case(shape, family, obj_kind):
    """(im [3,H,W], depth_sil [3,H,W], obj bytes [H,W])"""
    H, W = shape
    n = H * W
    rng = _rng(H, W, 100 + PENALTY_FAMILIES.index(family), PENALTY_OBJ.index(obj_kind))
    obj = make_obj(shape, obj_kind, seed=1)
    im = rng.uniform(-0.4, 1.0, (3, n)).astype(F)
    sil = rng.uniform(-0.2, 1.2, n).astype(F)
    flat = obj.reshape(-1)
    pick = lambda want: (np.flatnonzero(flat == want)[:1] if (flat == want).any() else np.array([0]))[0]
    if family == "zeros":
        im[rng.uniform(size=(3, n)) < 0.5] = 0.0
        im[0, 0] = -0.0
    elif family == "nan_inside":
        im[1, pick(1)] = np.nan
    elif family == "nan_outside":
        im[2, pick(0)] = np.nan
    elif family == "sil_edges":
        sil = rng.choice(np.array([-0.5, 0.0, -0.0, 1.0, 1.5, 0.3], F), n)
    elif family == "sil_nan":
        sil[pick(1)] = np.nan
    elif family == "sil_inf":
        sil[pick(0)] = np.inf
        sil[n - 1] = -np.inf
    ds = np.stack([rng.uniform(0.5, 5, n).astype(F), sil, rng.uniform(1, 30, n).astype(F)]).reshape(3, H, W)
    return np.ascontiguousarray(im.reshape(3, H, W)), np.ascontiguousarray(ds.astype(F)), obj


def make_outside_case(P, shape, cols, family, seed=0):
    """dict(means [P,3], logs [P,cols], w2c [4,4], K [3,3], obj [H,W] bytes); family 'exact' or 'general'"""
    H, W = shape
    rng = _rng(P, H, W, cols, 200 + (family == "general"), seed)
    obj = make_obj(shape, "half", seed=2 + seed)
    w2c = np.eye(4, dtype=F)
    if family == "exact":
        perm = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1)][(P + seed) % 4]
        R = np.zeros((3, 3), F)
        for r, c in enumerate(perm):
            R[r, c] = F(-1.0 if (r + seed) % 2 else 1.0)
        w2c[:3, :3] = R
        w2c[:3, 3] = np.array([1.0, -1.0, 2.0], F)
        means = (rng.integers(-256, 257, (P, 3)) / 64.0).astype(F)          # multiples of 2^-6 in [-4, 4]
        K = np.array([[32.0, 0, W // 2], [0, 32.0, H // 2], [0, 0, 1]], F)
    else:
        q = rng.normal(size=4)
        quat = (1.7 * q / np.linalg.norm(q)).astype(F)                       # unnormalised, as the optimiser leaves it
        w2c[:3, :3] = rotation_of(quat.astype(np.float64)).astype(F)
        w2c[:3, 3] = np.array([0.3, -0.2, 1.0], F)
        means = rng.uniform(-4, 4, (P, 3)).astype(F)
        f = 40.0 if shape == (48, 64) else 30.0
        K = np.array([[f, 0, W / 2 - 0.5], [0, f, H / 2 - 0.5], [0, 0, 1]], F)
    logs = rng.normal(-3.0, 1.0, (P, cols)).astype(F)
    case = dict(means=means, logs=logs, w2c=w2c, K=K, obj=obj)
    if family == "general":
        case["quat"] = quat
    return case


def rotation_of(q):
    """the rotation of the quaternion q = (r, x, y, z), normalised first (the reference's build_rotation), in q's precision"""
    r, x, y, z = q / np.sqrt((q * q).sum())
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                     [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                     [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])


def trajectory_params(case, frames=3, t=1):
    """torch `params` whose frame `t` has the case's pose: what get_gaussians_outside_mask reads (general family only)"""
    import torch
    rots = np.tile(np.array([1.0, 0, 0, 0], F)[None, :, None], (1, 1, frames))
    rots[0, :, t] = case["quat"]
    trans = np.zeros((1, 3, frames), F)
    trans[0, :, t] = case["w2c"][:3, 3]
    return dict(means3D=torch.from_numpy(case["means"]), log_scales=torch.from_numpy(case["logs"]),
                cam_unnorm_rots=torch.from_numpy(rots), cam_trans=torch.from_numpy(trans))


# ---- the cases of tests/golden/reference_object_loss.npz (make_reference_object_loss_vectors.py) ----------------------------------

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_object_loss.npz")
GOLDEN_LOSS_CASES = [("half", (16, 16), True), ("plateau", (37, 53), True), ("sil_at_thres", (5, 7), False)]   # family, shape, ignore_outlier_depth_loss
GOLDEN_OUTSIDE_CASES = [(4096, (48, 64), 3), (65, (37, 53), 1), (63, (37, 53), 3)]                              # P, mask, scale columns
GOLDEN_WEIGHTS = dict(im=0.5, depth=1.0)
GOLDEN_FRAME = 1


def make_golden_loss_case(i):
    """dict(im, gt_im [3,H,W], depth_sil [3,H,W], gt [1,H,W], obj bytes [H,W], ignore): one frame of the golden get_loss runs"""
    family, shape, ignore = GOLDEN_LOSS_CASES[i]
    H, W = shape
    ds, gt = make_mask_case(shape, family)
    rng = _rng(H, W, 300 + i)
    return dict(im=rng.uniform(-0.05, 1.05, (3, H, W)).astype(F), gt_im=rng.uniform(0, 1, (3, H, W)).astype(F), depth_sil=ds, gt=gt,
                obj=make_obj(shape, "half", seed=5 + i), ignore=ignore)


def make_golden_outside_case(i):
    P, shape, cols = GOLDEN_OUTSIDE_CASES[i]
    return make_outside_case(P, shape, cols, "general", seed=10 + i)


# ---- restatements ---------------------------------------------------------------------------------------------------------------

def mask_numpy(ds, gt, sil_thres, reject, presence, obj):
    """(mask bool [H,W], median bits) of the rule in NumPy binary32, in this helper's own form"""
    d, sil, d2 = ds[0].astype(F), ds[1].astype(F), ds[2].astype(F)
    g = gt[0].astype(F)
    keep = g > 0
    bits = 0
    with np.errstate(invalid="ignore", over="ignore"):
        if reject:
            err = (np.abs(g - d) * (g > 0).astype(F)).astype(F)
            flat = err.reshape(-1)
            med = F(np.nan) if np.isnan(flat).any() else np.sort(flat)[(flat.size - 1) // 2]
            bits = NAN_BITS if np.isnan(med) else int(np.array(med, F).view(np.uint32))
            keep = keep & (err < F(F(RATIO) * med))
        keep = keep & ~np.isnan(d) & ~np.isnan((d2 - (d * d).astype(F)).astype(F))
    if presence:
        keep = keep & (sil > F(sil_thres))
    if obj is not None:
        keep = keep & (obj != 0)
    return keep, bits


def mask_torch(ds, gt, sil_thres, reject, presence, obj):
    """(mask bool [H,W], median bits) from the torch chain on the CPU: `_loss_pixel_mask` and the object AND of the reference's
    gaussian_object.py:236-248 written out"""
    import torch
    from models.SLAM.gaussian import _loss_pixel_mask
    dst, gtt = torch.from_numpy(ds), torch.from_numpy(gt)
    _, keep = _loss_pixel_mask(dst, gtt, sil_thres, reject, presence)
    if obj is not None:
        keep = keep & torch.from_numpy(obj).bool().unsqueeze(0)
    bits = 0
    if reject:
        med = ((gtt - dst[0:1]).abs() * (gtt > 0)).median()
        bits = NAN_BITS if bool(torch.isnan(med)) else int(med.numpy().view(np.uint32))
    return keep[0].numpy(), bits


def penalty_torch(im, ds, obj, dtype, upstream=UPSTREAM):
    """(value, d/d im, d/d depth_sil) of upstream * (0.1 L_bg_rgb + 0.1 L_bg_alpha) by the reference's lines (gaussian_object.py:263-275,
    as `_background_penalty_torch` of models/SLAM/gaussian.py writes them) under torch autograd on the CPU, in `dtype`"""
    import torch
    from models.SLAM.gaussian import _background_penalty_torch
    a = torch.from_numpy(im).to(dtype).requires_grad_(True)
    b = torch.from_numpy(ds).to(dtype).requires_grad_(True)
    v = _background_penalty_torch(a, b[1], torch.from_numpy(obj).bool(), LAMBDA, LAMBDA)
    (v * upstream).backward()
    return float(v.detach()), a.grad.numpy(), b.grad.numpy()


def value_need(value, v32, v64):
    """deviation from the binary64 run / the rule's bound (tests/loss_cases.py `tolerance`): 2 D_ref + 64 2^-24 |value|, D_ref the
    binary32 torch chain's own deviation; a NaN reference needs a NaN"""
    if np.isnan(v64):
        return 0.0 if np.isnan(value) else np.inf
    tol = 2.0 * abs(float(v32) - float(v64)) + 64.0 * 2.0 ** -24 * abs(float(v64))
    dev = abs(float(value) - float(v64))
    return dev / tol if tol > 0 else (0.0 if dev == 0 else np.inf)


def outside_torch(case, dtype):
    """The reference's chain (slam_external.py:290-315) on the CPU in `dtype`: dict(outside, u, v, z, stats words as the status has them)"""
    import torch
    means, logs = torch.from_numpy(case["means"]).to(dtype), torch.from_numpy(case["logs"])
    w2c, K = torch.from_numpy(case["w2c"]).to(dtype), torch.from_numpy(case["K"]).to(dtype)
    obj = torch.from_numpy(case["obj"]).bool()
    H, W = obj.shape
    means_cam = (w2c[:3, :3] @ means.T + w2c[:3, 3:4]).T
    z = means_cam[:, 2]
    p = (K @ means_cam.T).T
    u = p[:, 0] / p[:, 2].clamp_min(1e-6)
    v = p[:, 1] / p[:, 2].clamp_min(1e-6)
    in_img = (z > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    iu = u[in_img].round().long().clamp(0, W - 1)
    iv = v[in_img].round().long().clamp(0, H - 1)
    inside = torch.zeros(means.shape[0], dtype=torch.bool)
    inside[in_img] = obj[iv, iu]
    outside = ~inside
    scale_max = torch.exp(logs).max(dim=1).values

    def rng(x):
        return (float("nan"), float("nan")) if x.numel() == 0 else (x.min().item(), x.max().item())
    words = [int(inside.sum()), int(outside.sum())] + [int(np.array(x, F).view(np.uint32)) if not np.isnan(x) else NAN_BITS
                                                       for x in rng(scale_max[inside]) + rng(scale_max[outside])]
    return dict(outside=outside.numpy(), u=u.numpy(), v=v.numpy(), z=z.numpy(), status=np.array(words, np.int64))


def exp_is_correctly_rounded(logs):
    """where torch's binary32 exp is the correctly rounded one (the header's, through binary64): the status words of the exact
    family are compared bit for bit, so its log scales are drawn where the two agree"""
    import torch
    return torch.exp(torch.from_numpy(logs)).numpy() == np.exp(logs.astype(np.float64)).astype(F)


# ---- the g++ harness over csrc/fr_objloss_math.h (tests/harness/fr_objloss_harness.cpp) --------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_objloss_harness"))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.fro_loss_mask.argtypes = [ci, ci, cf, ci, cf, ci] + [vp] * 5
    h.fro_penalty_forward.argtypes = [ci, ci, cf, cf] + [vp] * 5
    h.fro_penalty_backward.argtypes = [ci, ci, cf, cf] + [vp] * 4 + [cf, vp, vp]
    h.fro_outside_mask.argtypes = [ci, ci] + [vp] * 5 + [ci, ci, vp, vp]
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def harness_mask(h, ds, gt, sil_thres, reject, presence, obj):
    """(mask bytes [H,W], status int32 [5])"""
    H, W = ds.shape[1:]
    mask, status = np.zeros((H, W), np.uint8), np.zeros(5, np.int32)
    h.fro_loss_mask(H, W, sil_thres, int(reject), RATIO, int(presence), _ptr(ds), _ptr(gt), _ptr(obj), _ptr(mask), _ptr(status))
    return mask, status


def harness_penalty(h, im, ds, obj, upstream=UPSTREAM):
    """dict(out4, saved2, g_im, g_ds)"""
    H, W = obj.shape
    out4, saved2 = np.zeros(4, F), np.zeros(2, F)
    g_im, g_ds = np.zeros((3, H, W), F), np.zeros((3, H, W), F)
    h.fro_penalty_forward(H, W, LAMBDA, LAMBDA, _ptr(im), _ptr(ds), _ptr(obj), _ptr(out4), _ptr(saved2))
    h.fro_penalty_backward(H, W, LAMBDA, LAMBDA, _ptr(im), _ptr(ds), _ptr(obj), _ptr(saved2), upstream, _ptr(g_im), _ptr(g_ds))
    return dict(out4=out4, saved2=saved2, g_im=g_im, g_ds=g_ds)


def harness_outside(h, case):
    """(outside bytes [P], status int32 [6])"""
    P, cols = case["logs"].shape
    H, W = case["obj"].shape
    outside, status = np.zeros(P, np.uint8), np.zeros(6, np.int32)
    h.fro_outside_mask(P, cols, _ptr(case["means"]), _ptr(case["logs"]), _ptr(case["w2c"]), _ptr(case["K"]), _ptr(case["obj"]), H, W,
                       _ptr(outside), _ptr(status))
    return outside, status


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def load_golden():
    return np.load(GOLDEN)


# ---- the loss terms around the mask, restated in torch (the reference's calc_loss / calc_loss_mask, slam_helpers.py:23-77) --------

def _ssim_torch(x, y):
    import torch
    import torch.nn.functional as Fn
    from loss_cases import TAPS_BITS
    taps = torch.from_numpy(TAPS_BITS.view(np.float32).copy())
    w = (taps[:, None] * taps[None, :]).to(device=x.device, dtype=x.dtype).expand(3, 1, 11, 11).contiguous()
    blur = lambda a: Fn.conv2d(a[None], w, padding=5, groups=3)[0]
    mu1, mu2 = blur(x), blur(y)
    s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
    return (((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))).mean()


def torch_calc_loss(masked_mapping):
    """calc_loss (masked_mapping=False) or calc_loss_mask (True) as a torch chain, for the runs that have no kernels under them"""
    import torch

    def calc(curr, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking):
        terms = {}
        if use_l1:
            d = torch.abs(curr['depth'] - depth)[mask]
            terms['depth'] = d.sum() if tracking else d.mean()
        if tracking and (use_sil_for_loss or ignore_outlier_depth_loss):
            terms['im'] = torch.abs(curr['im'] - im)[color_mask].sum()
        elif tracking:
            terms['im'] = torch.abs(curr['im'] - im).sum()
        elif masked_mapping:
            m = color_mask.float()
            terms['im'] = 0.8 * torch.abs(im - curr['im'])[color_mask].mean() + 0.2 * (1.0 - _ssim_torch(im * m, curr['im'] * m))
        else:
            terms['im'] = 0.8 * torch.abs(im - curr['im']).mean() + 0.2 * (1.0 - _ssim_torch(im, curr['im']))
        return terms
    return calc


def grad_need(got, g32, g64):
    """largest deviation from the binary64 gradient / the rule's bound, 2 D_ref + 64 2^-24 max |gradient|"""
    g64 = np.asarray(g64, np.float64)
    tol = 2.0 * float(np.abs(np.asarray(g32, np.float64) - g64).max()) + 64.0 * 2.0 ** -24 * float(np.abs(g64).max())
    dev = float(np.abs(np.asarray(got, np.float64) - g64).max())
    return dev / tol if tol > 0 else (0.0 if dev == 0 else np.inf)


def outside_band(u, v, z, W, H):
    """The Gaussians whose binary64 projection is too close to a decision to hold a binary32 chain to it: z within 1e-3 of 0, or, in
    front of the camera, u or v within 64 2^-24 (1 + |u| + |v|) of 0 / W / H or -- inside the image, where the pixel is looked up --
    of a half-integer.  (Behind the camera nothing depends on u and v, outside the image nothing on their rounding.)"""
    with np.errstate(invalid="ignore", over="ignore"):
        eps = 64.0 * 2.0 ** -24 * (1.0 + np.abs(u) + np.abs(v))
        edge = lambda a, hi: np.minimum(np.abs(a), np.abs(a - hi)) <= eps
        half = lambda a: np.abs((a - 0.5) - np.round(a - 0.5)) <= eps
        in_img = (u >= 0) & (u < W) & (v >= 0) & (v < H)
        return (np.abs(z) <= 1e-3) | ((z > 0) & (edge(u, float(W)) | edge(v, float(H)) | (in_img & (half(u) | half(v)))))
