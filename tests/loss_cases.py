"""Inputs, terms and a float64 NumPy restatement for the fused image loss (fr_image_loss_forward / _backward).

The cases are regenerated from seeds, not stored: `make_case(shape, family, mask_kind)` is what
tests/golden/make_reference_loss_vectors.py fed to the reference's own calc_ssim / calc_ssim_masked / calc_loss / calc_loss_mask
(binary32 and binary64, on the CPU) and what the tests feed to the harness and to the kernels.  `loss64` states the same loss and
its gradient w.r.t. the render in float64 NumPy, in this helper's own form, for the shapes that have no fixture; on the fixture's
cases it equals the reference's binary64 run to 1e-12 (tests/test_image_loss_cpu.py)."""
import os

import numpy as np
import harness_build

SHAPES = [(3, 11, 11), (3, 5, 70), (3, 17, 33), (1, 17, 33)]
FAMILIES = ["noise", "smooth", "flat", "step", "identical"]
MASK_KINDS = ["none", "half", "empty"]
L1_SUM, L1_MEAN, L1_MASKED_MEAN = 0, 1, 2

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_loss.npz")

# gaussian(11, 1.5) of the reference in binary32, as bits (recorded in the fixture as "taps_bits" and compared there)
TAPS_BITS = np.array([981912246, 1006173953, 1024685452, 1038088319, 1046093343, 1049113264,
                      1046093343, 1038088319, 1024685452, 1006173953, 981912246], dtype=np.uint32)


def _seed(shape, family, what):
    return [int(s) for s in shape] + [FAMILIES.index(family), what, 20240611]


def make_images(shape, family):
    """(render x, target y), float32 [C,H,W]"""
    C, H, W = shape
    rng = np.random.default_rng(_seed(shape, family, 0))
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if family == "noise":
        x, y = rng.uniform(0, 1, shape), rng.uniform(0, 1, shape)
    elif family == "smooth":
        ph = rng.uniform(0, 6.28, (C, 1, 1))
        y = 0.5 + 0.3 * np.sin(0.21 * xx[None] + 0.13 * yy[None] + ph)
        x = y + 0.05 * np.sin(0.37 * xx[None] - 0.29 * yy[None] + 2 * ph) + rng.normal(0, 2e-3, shape)
    elif family == "flat":                                  # 0.7 +- 0.003: sigma^2 cancels against c2
        x, y = 0.7 + rng.uniform(-0.003, 0.003, shape), 0.7 + rng.uniform(-0.003, 0.003, shape)
    elif family == "step":
        y = np.where(xx[None] < W // 2, 0.2, 0.8) + np.zeros(shape)
        x = np.where(xx[None] + (yy[None] > H // 2) < W // 2 + 1, 0.25, 0.75) + rng.normal(0, 1e-2, shape)
    elif family == "identical":
        y = rng.uniform(0, 1, shape)
        x = y.copy()
    else:
        raise ValueError(family)
    return x.astype(np.float32), y.astype(np.float32)


def make_masks(shape, family, mask_kind):
    """(mask1 [1,H,W] bool, mask_c [C,H,W] bool): the pixel mask and an independent per-channel colour mask"""
    C, H, W = shape
    rng = np.random.default_rng(_seed(shape, family, 1))
    if mask_kind == "none":
        return np.ones((1, H, W), bool), np.ones(shape, bool)
    if mask_kind == "empty":
        return np.zeros((1, H, W), bool), np.zeros(shape, bool)
    return rng.uniform(size=(1, H, W)) < 0.5, rng.uniform(size=shape) < 0.5


def make_case(shape, family, mask_kind):
    x, y = make_images(shape, family)
    m1, mc = make_masks(shape, family, mask_kind)
    return x, y, m1, mc


class Term:
    """One loss term as the kernels see it; `mask` names which mask it takes ('none', '1' = [1,H,W], 'c' = [C,H,W]) and `out`
    which of out4 is the value ('loss' or 'ssim': with w_l1 = 0, w_ssim = -1 the loss is ssim - 1 and the value the SSIM mean)."""

    def __init__(self, name, w_l1, w_ssim, denom, mask="none", weights_map=False, out="loss"):
        self.name, self.w_l1, self.w_ssim, self.denom, self.mask, self.weights_map, self.out = name, w_l1, w_ssim, denom, mask, weights_map, out

    def pick_mask(self, m1, mc):
        return None if self.mask == "none" else (m1 if self.mask == "1" else mc)

    def grad_floor(self, n):
        """(w_l1 + w_ssim) / (C H W) of the tolerance rule"""
        return (abs(self.w_l1) + abs(self.w_ssim)) / n


def terms_for(C, mask_kind):
    """The reference's branches a case exercises: colour terms for C = 3, depth terms for C = 1."""
    if C == 1:           # depth (mask "none" is the full mask): masked mean in mapping, masked sum in tracking
        return [Term("map_depth", 1.0, 0.0, L1_MASKED_MEAN, "1"), Term("trk_depth", 1.0, 0.0, L1_SUM, "1")]
    if mask_kind == "none":
        return [Term("ssim", 0.0, -1.0, L1_SUM, out="ssim"), Term("map_im", 0.8, 0.2, L1_MEAN), Term("trk_im", 1.0, 0.0, L1_SUM)]
    return [Term("ssim_masked", 0.0, -1.0, L1_SUM, "1", True, "ssim"), Term("trk_im_masked", 1.0, 0.0, L1_SUM, "c"),
            Term("mapmask_im", 0.8, 0.2, L1_MASKED_MEAN, "c")]


def all_cases():
    for shape in SHAPES:
        for family in FAMILIES:
            for kind in MASK_KINDS:
                yield shape, family, kind


def key(shape, family, kind, term):
    return f"{shape[0]}x{shape[1]}x{shape[2]}/{family}/{kind}/{term}"


def tolerance(term, n, ref_loss32, ref_loss64, grad64, grad_dev32):
    """The rule: within 2 D_ref + 64 2^-24 scale of the binary64 run; D_ref = the reference's own binary32 deviation."""
    eps = 64.0 * 2.0 ** -24
    loss_tol = 2.0 * abs(float(ref_loss32) - float(ref_loss64)) + eps * abs(float(ref_loss64))
    grad_tol = 2.0 * float(grad_dev32) + eps * max(float(np.abs(grad64).max()), term.grad_floor(n))
    return loss_tol, grad_tol


def needs(term, n, value, grad, ref_loss32, ref_loss64, grad64, grad_dev32):
    """(loss need, gradient need) = deviation from the binary64 run / the rule's bound; a NaN reference value (the masked mean of
    an empty mask) needs a NaN"""
    loss_tol, grad_tol = tolerance(term, n, ref_loss32, 0.0 if np.isnan(ref_loss64) else ref_loss64, grad64, grad_dev32)
    if np.isnan(ref_loss64):
        lneed = 0.0 if np.isnan(value) else np.inf
    else:
        dev = abs(float(value) - float(ref_loss64))
        lneed = dev / loss_tol if loss_tol > 0 else (0.0 if dev == 0 else np.inf)
    gerr = float(np.abs(np.asarray(grad, np.float64).reshape(-1) - np.asarray(grad64, np.float64).reshape(-1)).max())
    return lneed, gerr / grad_tol


# ---- the float64 restatement ---------------------------------------------------------------------------------------------------

def window2d():
    """The 11 x 11 window the reference builds: the binary32 outer product of the binary32 taps (each entry one rounding)"""
    g = TAPS_BITS.view(np.float32)
    return (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)


def _filter(a, w):
    """zero-padded 11 x 11 correlation of every channel of a [C,H,W]"""
    C, H, W = a.shape
    p = np.zeros((C, H + 10, W + 10))
    p[:, 5:5 + H, 5:5 + W] = a
    out = np.zeros((C, H, W))
    for i in range(11):
        for j in range(11):
            out += w[i, j] * p[:, i:i + H, j:j + W]
    return out


def loss64(x, y, mask, w_l1, w_ssim, denom, weights_map=False):
    """(out4 = [loss, l1 term, ssim mean, count], d loss / d x) in float64.  mask: bool [C,H,W] / [1,H,W] or None."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    C, H, W = x.shape
    n = C * H * W
    m = np.ones((C, H, W)) if mask is None else np.broadcast_to(np.asarray(mask, np.float64), (C, H, W))
    count = float(m.sum())
    sel = m if not weights_map else np.ones((C, H, W))          # what selects the L1 pixels and multiplies the images
    grad = np.zeros((C, H, W))
    l1_den = 1.0 if denom == L1_SUM else (float(n) if denom == L1_MEAN else count)
    with np.errstate(divide="ignore", invalid="ignore"):
        l1 = float((np.abs(x - y) * sel).sum()) / l1_den if l1_den != 0 else float("nan")
    if w_l1 != 0 and l1_den != 0:
        grad += w_l1 / l1_den * np.sign(x - y) * sel
    ssim = 0.0
    if w_ssim != 0:
        w = window2d()
        xm, ym = x * sel, y * sel
        mu1, mu2 = _filter(xm, w), _filter(ym, w)
        e11, e22, e12 = _filter(xm * xm, w), _filter(ym * ym, w), _filter(xm * ym, w)
        s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
        A1, A2 = 2 * mu1 * mu2 + 0.01 ** 2, 2 * s12 + 0.03 ** 2
        B1, B2 = mu1 * mu1 + mu2 * mu2 + 0.01 ** 2, s1 + s2 + 0.03 ** 2
        smap = A1 * A2 / (B1 * B2)
        wgt = m if weights_map else np.ones((C, H, W))
        norm = max(count, float(C)) if weights_map else float(n)
        ssim = float((smap * wgt).sum()) / norm
        d11 = -smap / B2 * wgt
        d12 = 2 * A1 / (B1 * B2) * wgt
        dmu = (2 * mu2 * (A2 - A1) / (B1 * B2) + 2 * mu1 * smap * (1 / B2 - 1 / B1)) * wgt
        grad += -w_ssim / norm * (_filter(dmu, w) + 2 * xm * _filter(d11, w) + ym * _filter(d12, w)) * sel
    loss = (w_l1 * l1 if w_l1 != 0 else 0.0) + (w_ssim * (1.0 - ssim) if w_ssim != 0 else 0.0)
    return np.array([loss, l1, ssim, count]), grad


# ---- the g++ harness over csrc/fr_loss_math.h (tests/harness/fr_loss_harness.cpp) ----------------------------------------------

def build_harness():
    """ctypes handle of the harness, built with the flags conftest.py uses for the other one"""
    import ctypes
    h = ctypes.CDLL(harness_build.shared("fr_loss_harness"))
    h.frl_sign_of.restype = ctypes.c_float
    h.frl_sign_of.argtypes = [ctypes.c_float]
    vp = ctypes.c_void_p
    h.frl_forward.argtypes = [ctypes.c_int] * 3 + [ctypes.c_float] * 2 + [ctypes.c_int] * 3 + [vp] * 7
    h.frl_backward.argtypes = [ctypes.c_int] * 3 + [ctypes.c_float] + [ctypes.c_int] * 2 + [vp] * 4 + [ctypes.c_float, vp]
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def harness_forward(h, x, y, mask, w_l1, w_ssim, denom, weights_map=False):
    """dict(out = float64 [4], channel_ssim = float64 [C], ssim_map, saved (with its 4-float tail)) from the harness"""
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    C, H, W = x.shape
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    ssim = float(w_ssim) != 0.0
    out, chan = np.zeros(4), np.zeros(C)
    smap = np.zeros((C, H, W), np.float32) if ssim else None
    saved = np.zeros((3 * C * H * W if ssim else 0) + 4, np.float32)
    h.frl_forward(C, H, W, w_l1, w_ssim, denom, 0 if m is None else m.shape[0], int(weights_map), _ptr(x), _ptr(y), _ptr(m),
                  _ptr(out), _ptr(chan), _ptr(smap), _ptr(saved))
    return dict(out=out, channel_ssim=chan, ssim_map=smap, saved=saved)


def harness_backward(h, x, y, mask, w_ssim, saved, upstream, weights_map=False):
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    C, H, W = x.shape
    m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    g = np.zeros((C, H, W), np.float32)
    h.frl_backward(C, H, W, w_ssim, 0 if m is None else m.shape[0], int(weights_map), _ptr(x), _ptr(y), _ptr(m), _ptr(saved),
                   upstream, _ptr(g))
    return g


def load_fixture():
    """{key: (value32, value64, grad deviation32, grad64 flat float32)} and the taps' bits from tests/golden/reference_loss.npz"""
    z = np.load(FIXTURE)
    off = z["offsets"]
    return {str(k): (z["values"][i, 0], z["values"][i, 1], z["values"][i, 2], z["grad64"][off[i]:off[i + 1]])
            for i, k in enumerate(z["keys"])}, z["taps_bits"]
