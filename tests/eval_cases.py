"""Inputs, the tolerance rule and the harness binding for the render-quality evaluation (fr_view_metrics).

The cases are regenerated from seeds, not stored: `make_batch(shape, rot, mask_kind)` is what
tests/golden/make_reference_eval_vectors.py fed to the reference's own calc_psnr / calc_ssim (binary32 and binary64, on the CPU)
and what the tests feed to the harness and to the kernels.  Every batch mixes families across its views -- view v is of family
FAMILIES[(v + rot) % 7] -- so a wrong view stride shows as a wrong number.  A target is always an image of bytes (Habitat's rgb):
its float form is bytes / 255 in binary32, so the three target layouts state the same image."""
import ctypes
import os

import numpy as np
import harness_build

SHAPES = [(1, 11, 11), (3, 5, 70), (5, 17, 33), (2, 16, 16)]
FAMILIES = ["noise", "smooth", "step", "identical", "near", "out_of_range", "black_gt"]
LAYOUTS = ["f32", "u8x3", "u8x4"]
MASK_KINDS = ["none", "half", "empty"]
ROW = 8
PSNR, SSIM, DEPTH_L1, DEPTH_RMSE, MSE_R, MSE_G, MSE_B, DEPTH_COUNT = range(8)
# the reference's values per view in the fixture: colour, then the depth terms over all pixels and over the valid ones
REF_NAMES = ["psnr", "ssim", "l1_all", "rmse_all", "l1_valid", "rmse_valid"]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_eval.npz")


def _seed(hw, family, what):
    return [int(hw[0]), int(hw[1]), FAMILIES.index(family), what, 20240917]


def make_view(hw, family, v):
    """(render float32 [3,H,W], target bytes uint8 [H,W,3], depth float32 [H,W], gt_depth float32 [H,W]) of one view"""
    H, W = hw
    rng = np.random.default_rng(_seed(hw, family, v))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    shape = (3, H, W)
    if family == "noise":
        y = rng.uniform(0, 1, shape)
    elif family == "smooth":
        ph = rng.uniform(0, 6.28, (3, 1, 1))
        y = 0.5 + 0.3 * np.sin(0.21 * xx[None] + 0.13 * yy[None] + ph)
    elif family == "step":
        y = np.where(xx[None] < W // 2, 0.2, 0.8) + np.zeros(shape)
    elif family == "black_gt":
        y = np.zeros(shape)
    else:
        y = rng.uniform(0, 1, shape)
    gt_u8 = np.ascontiguousarray(np.clip(np.rint(y * 255), 0, 255).astype(np.uint8).transpose(1, 2, 0))
    y = u8_to_f32(gt_u8)
    if family == "noise":
        x = rng.uniform(0, 1, shape)
    elif family == "smooth":
        x = y + 0.05 * np.sin(0.37 * xx[None] - 0.29 * yy[None]) + rng.normal(0, 2e-3, shape)
    elif family == "step":
        x = np.where(xx[None] + (yy[None] > H // 2) < W // 2 + 1, 0.25, 0.75) + rng.normal(0, 1e-2, shape)
    elif family == "identical":
        x = y.copy()
    elif family == "near":
        x = y + rng.normal(0, 1e-4, shape)
    elif family == "out_of_range":
        x = rng.uniform(-0.3, 1.3, shape)
    else:                                                       # black_gt
        x = rng.uniform(0, 0.2, shape)
    gt_depth = rng.uniform(0.5, 4.0, (H, W))
    gt_depth[rng.uniform(size=(H, W)) < 1.0 / 3.0] = 0.0         # a third of the pixels has no measured depth
    if family == "black_gt":
        gt_depth[:] = 0.0                                       # and this view none at all: the valid-only terms are 0 / 0
    depth = gt_depth + rng.normal(0, 0.05, (H, W)) + (gt_depth == 0) * rng.uniform(0.5, 4.0, (H, W))
    return x.astype(np.float32), gt_u8, depth.astype(np.float32), gt_depth.astype(np.float32)


def u8_to_f32(gt_u8):
    """bytes [..., H, W, 3|4] -> float32 [..., 3, H, W], value / 255 in binary32 (one correctly rounded division)"""
    f = gt_u8[..., :3].astype(np.float32) / np.float32(255.0)
    return np.ascontiguousarray(np.moveaxis(f, -1, -3))


def make_batch(shape, rot, mask_kind):
    V, H, W = shape
    fams = [FAMILIES[(v + rot) % len(FAMILIES)] for v in range(V)]
    views = [make_view((H, W), f, v) for v, f in enumerate(fams)]
    rng = np.random.default_rng([V, H, W, rot, MASK_KINDS.index(mask_kind), 77])
    gt_u8 = np.stack([t[1] for t in views])
    alpha = rng.integers(0, 256, (V, H, W, 1), dtype=np.uint8)          # the fourth channel: garbage that must not matter
    if mask_kind == "none":
        mask = None
    elif mask_kind == "empty":
        mask = np.zeros((V, H, W), np.uint8)
    else:
        mask = (rng.uniform(size=(V, H, W)) < 0.5).astype(np.uint8)
    return dict(shape=shape, families=fams, render=np.stack([t[0] for t in views]), gt_u8=gt_u8, gt_f32=u8_to_f32(gt_u8),
                gt_u8x4=np.ascontiguousarray(np.concatenate((gt_u8, alpha), axis=-1)), mask=mask,
                depth=np.stack([t[2] for t in views]), gt_depth=np.stack([t[3] for t in views]))


def target_of(batch, layout):
    return {"f32": batch["gt_f32"], "u8x3": batch["gt_u8"], "u8x4": batch["gt_u8x4"]}[layout]


def all_cases():
    """(shape, rot, mask kind, clamp): every family meets every shape and every mask; without the clamp where it matters"""
    for shape in SHAPES:
        for rot in range(len(FAMILIES)):
            for kind in MASK_KINDS:
                yield shape, rot, kind, True
            if "out_of_range" in [FAMILIES[(v + rot) % len(FAMILIES)] for v in range(shape[0])]:
                yield shape, rot, "none", False
                yield shape, rot, "half", False


def key(shape, rot, kind, clamp):
    return f"{shape[0]}x{shape[1]}x{shape[2]}/{rot}/{kind}/{'clamp' if clamp else 'raw'}"


def load_fixture():
    """{key: float64 [V, 2, 6]}: per view the reference's binary32 and binary64 values of REF_NAMES"""
    z = np.load(FIXTURE)
    off = z["offsets"]
    return {str(k): z["values"][off[i]:off[i + 1]] for i, k in enumerate(z["keys"])}


def need(value, ref32, ref64):
    """deviation / bound under the project's rule: within 2 D_ref + 64 2^-24 |value| of the reference's binary64 run, D_ref the
    deviation of its own binary32 run.  An infinite reference needs the same infinity and a NaN needs a NaN (need 0 or inf)."""
    value, ref32, ref64 = float(value), float(ref32), float(ref64)
    if np.isnan(ref64):
        return 0.0 if np.isnan(value) else np.inf
    if np.isinf(ref64):
        return 0.0 if value == ref64 else np.inf
    if not np.isfinite(value):
        return np.inf
    d_ref = abs(ref32 - ref64) if np.isfinite(ref32) else 0.0
    bound = 2.0 * d_ref + 64.0 * 2.0 ** -24 * abs(ref64)
    dev = abs(value - ref64)
    return dev / bound if bound > 0 else (0.0 if dev == 0 else np.inf)


def row_refs(ref_view, valid_only):
    """[(row index, ref32, ref64)] of one view's fixture entry [2, 6] for the four metrics of a row"""
    d = 4 if valid_only else 2
    return [(PSNR, ref_view[0, 0], ref_view[1, 0]), (SSIM, ref_view[0, 1], ref_view[1, 1]),
            (DEPTH_L1, ref_view[0, d], ref_view[1, d]), (DEPTH_RMSE, ref_view[0, d + 1], ref_view[1, d + 1])]


def summary64(rows):
    """the summary restated in NumPy over float32 rows [V, 8]: the keep rule is `not isinf(psnr)`, the means are float64"""
    rows = np.asarray(rows, np.float32)
    kept = ~np.isinf(rows[:, PSNR])
    out = np.zeros(ROW)
    out[0], out[7] = kept.sum(), rows.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        for k in range(4):
            out[1 + k] = np.float64(rows[kept, k].astype(np.float64).sum()) / np.float64(kept.sum())
    return out


def ulp_diff(a, b):
    """distance in binary32 ulps between float32 arrays (0 where both are NaN or the same infinity; huge where only one is)"""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    out = np.zeros(a.shape, np.float64)
    for i, (p, q) in enumerate(zip(a, b)):
        if np.isnan(p) or np.isnan(q):
            out[i] = 0 if (np.isnan(p) and np.isnan(q)) else np.inf
        elif np.isinf(p) or np.isinf(q):
            out[i] = 0 if p == q else np.inf
        else:
            ip, iq = int(np.float32(p).view(np.int32)), int(np.float32(q).view(np.int32))
            ip = ip if ip >= 0 else -(ip & 0x7FFFFFFF)
            iq = iq if iq >= 0 else -(iq & 0x7FFFFFFF)
            out[i] = abs(ip - iq)
    return out


# ---- the g++ harness over csrc/fr_eval_math.h (tests/harness/fr_eval_harness.cpp) ----------------------------------------------

def build_harness():
    """ctypes handle of the harness, built with the flags loss_cases.build_harness uses"""
    h = ctypes.CDLL(harness_build.shared("fr_eval_harness"))
    vp, ll = ctypes.c_void_p, ctypes.c_longlong
    h.fre_clamp_of.restype = ctypes.c_float
    h.fre_clamp_of.argtypes = [ctypes.c_float]
    h.fre_byte_table.argtypes = [vp]
    h.fre_summary.argtypes = [vp, ctypes.c_int, vp]
    h.fre_view_metrics.argtypes = [ctypes.c_int] * 7 + [vp, ll, vp, ll, vp, vp, ll, vp, vp, vp]
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def harness_metrics(h, render, gt, depth=None, gt_depth=None, mask=None, clamp=True, valid_only=False):
    """(rows float32 [V,8], summary float32 [8]) from the harness; gt: float32 [V,3,H,W] or uint8 [V,H,W,3|4]"""
    render = np.ascontiguousarray(render, np.float32)
    V, _, H, W = render.shape
    u8 = gt.dtype == np.uint8
    gt = np.ascontiguousarray(gt)
    depth = None if depth is None else np.ascontiguousarray(depth, np.float32)
    gt_depth = None if gt_depth is None else np.ascontiguousarray(gt_depth, np.float32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    rows, summary = np.zeros((V, ROW), np.float32), np.zeros(ROW, np.float32)
    h.fre_view_metrics(V, H, W, int(u8), int(gt.shape[-1]) if u8 else 3, int(clamp), int(valid_only), _ptr(render), 3 * H * W,
                       _ptr(depth), H * W, _ptr(gt), _ptr(gt_depth), H * W, _ptr(mask), _ptr(rows), _ptr(summary))
    return rows, summary


def harness_summary(h, rows):
    rows = np.ascontiguousarray(rows, np.float32)
    out = np.zeros(ROW, np.float32)
    h.fre_summary(_ptr(rows), rows.shape[0], _ptr(out))
    return out
