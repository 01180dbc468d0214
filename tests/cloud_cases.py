"""Cases of the nearest-point search (fr_cloud_query): seeded generators, the SciPy float64 statement, the qualification checks, and
the g++ harness over csrc/fr_cloud_math.h (tests/harness/fr_cloud_harness.cpp) -- the bit-exact statement of what the kernels return.

Qualification (a condition on a case, not on the code): a case compared with the float64 statement or with the outputs of the
reference's own functions (tests/golden/reference_cloud.npz) has no float64 nearest distance within relative 1e-5 of dist_th in
"points" mode, none within 1e-4 m of it in "depth" mode, and coordinates below 16 m.  binary32 spacing at 16 m is 1.9e-6 m and the
reference's torch matmul orders its sums differently; the margins are 50 times that, so no flag can differ.  `qualifying_*` search
seeds until a case qualifies."""
import ctypes
import os

import numpy as np
import harness_build

F = np.float32
FAMILIES = ("uniform", "clusters", "outside", "plane", "point", "surface", "nonfinite")
N_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)          # wave, sub-box, box and sort-chunk edges
N_LARGE = 40000
M_SIZES = (1, 63, 64, 65, 257, 1000)
THRESHOLDS = (0.05, 0.01)
MAX_SEEDS = 64
COORD_LIMIT = 16.0
REL_MARGIN = 1e-5
DEPTH_MARGIN = 1e-4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- "points" cases -------------------------------------------------------------------------------------------------------------------

def make_case(family, N, M, seed=0):
    """(targets [N,3], queries [M,3]) float32"""
    rng = np.random.default_rng([FAMILIES.index(family), N, M, seed])
    t = rng.uniform(-4, 4, (N, 3))
    q = rng.uniform(-4, 4, (M, 3))
    if family == "clusters":
        # a quarter of the targets in a cube of 1/400 of the volume (100 x the density), exact duplicates, queries equal to targets
        k = N // 4
        t[:k] = rng.uniform(1.0, 1.0 + 8 / 400 ** (1 / 3), (k, 3))
        if N >= 2:
            dup = rng.integers(0, N, max(1, N // 8))
            t[dup] = t[(dup + 1) % N]
        hit = rng.uniform(size=M) < 0.5
        q[hit] = t[rng.integers(0, N, int(hit.sum()))]
    elif family == "outside":
        t = rng.uniform(-2, 2, (N, 3))
        far = np.arange(M) % 2 == 1
        q[far] = rng.uniform(8, 15, (int(far.sum()), 3)) * rng.choice([-1.0, 1.0], (int(far.sum()), 3))
    elif family == "plane":
        t[:, rng.integers(0, 3)] = 1.25
    elif family == "point":
        t[:] = rng.uniform(-4, 4, 3)
    elif family == "surface":
        q = t[rng.integers(0, N, M)] + rng.normal(0, 0.03, (M, 3))
    t, q = t.astype(F), q.astype(F)
    if family == "nonfinite":
        bad = np.array([np.nan, np.inf, -np.inf], F)
        for a in (t, q):
            n = max(1, a.shape[0] // 20)
            a[rng.integers(0, a.shape[0], n), rng.integers(0, 3, n)] = bad[rng.integers(0, 3, n)]
    return t, q


def scipy_nearest(targets, queries):
    """the float64 statement: (distances [M] float64 -- +inf without a finite target, NaN for a non-finite query --, indices)"""
    from scipy.spatial import KDTree
    t64, q64 = np.asarray(targets, np.float64), np.asarray(queries, np.float64)
    tf, qf = np.isfinite(t64).all(1), np.isfinite(q64).all(1)
    d = np.full(len(q64), np.nan)
    i = np.full(len(q64), -1, np.int64)
    if tf.any() and qf.any():
        dd, ii = KDTree(t64[tf]).query(q64[qf])
        d[qf], i[qf] = dd, np.flatnonzero(tf)[ii]
    elif qf.any():
        d[qf] = np.inf
    return d, i


def qualifies_points(targets, queries, thresholds=THRESHOLDS, d64=None):
    d = scipy_nearest(targets, queries)[0] if d64 is None else d64
    d = d[np.isfinite(d)]
    for a in (targets, queries):
        a = np.asarray(a)
        if a.size and np.abs(a[np.isfinite(a)]).max(initial=0.0) >= COORD_LIMIT:
            return False
    return all(not (np.abs(d - th) <= REL_MARGIN * th).any() for th in thresholds)


def qualifying_case(family, N, M):
    for seed in range(MAX_SEEDS):
        t, q = make_case(family, N, M, seed)
        if qualifies_points(t, q):
            return t, q, seed
    raise AssertionError(f"no qualifying seed for {family} N={N} M={M}")


def scipy_metrics(gt, rec, dist_th):
    """what accuracy_comp_ratio_from_pcl computes, from the float64 statement (finite clouds)"""
    d_rec = scipy_nearest(gt, rec)[0]
    d_gt = scipy_nearest(rec, gt)[0]
    return float(np.mean(d_rec)), float(np.mean(d_gt)), float(np.mean((d_gt < dist_th).astype(float)))


# ---- "depth" cases --------------------------------------------------------------------------------------------------------------------

DEPTH_SHAPES = ((48, 64), (47, 63))
DEPTH_KINDS = ("object", "few", "none-valid")


def _rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    c2w = np.eye(4)
    c2w[:3, :3], c2w[:3, 3] = q, rng.uniform(-2, 2, 3)
    return c2w


def make_depth_case(H, W, kind="object", z_forward="-Z", seed=0):
    """A wall 2.5 m in front of a camera of random pose; the environment cloud is the wall sampled every 2 cm (so an observed wall
    point is within about 1.5 cm of it); an object 1 m in front of the wall is not in the cloud: its pixels are novel.  `few`: an
    object of 4 x 4 pixels (1 to 19 novel samples at any stride); `none-valid`: no pixel has a depth.  The depth also holds 0,
    negative, inf and NaN pixels."""
    rng = np.random.default_rng([H, W, DEPTH_KINDS.index(kind), z_forward == "-Z", seed])
    fx = 50.0
    K = np.array([[fx, 0, W / 2 - 0.5], [0, fx, H / 2 - 0.5], [0, 0, 1]])
    inv_K = np.eye(4)
    inv_K[:3, :3] = np.linalg.inv(K)
    c2w = _rigid(rng)
    sign = -1.0 if z_forward in ("-Z", "-z") else 1.0
    depth = 2.5 + rng.uniform(-0.004, 0.004, (H, W))
    if kind == "object":
        depth[H // 4:H // 2, W // 4:W // 2] = 1.5
    elif kind == "few":
        depth[9:13, 18:22] = 1.5
    n_bad = H * W // 16
    depth.reshape(-1)[rng.integers(0, H * W, n_bad)] = np.array([0.0, -1.0, np.inf, np.nan])[rng.integers(0, 4, n_bad)]
    depth[H - 1, W - 1] = 2.5                                  # the last pixel has a depth
    depth[16:24, 8:16] = 0.0                                   # an 8 x 8 block (at stride 1) without any
    if kind == "none-valid":
        depth = np.where(rng.uniform(size=(H, W)) < 0.5, 0.0, np.nan)
    # the wall in the camera frame, a little beyond the image on every side, every 2 cm
    xs = np.arange(-(W / 2 + 2) / fx * 2.5, (W / 2 + 2) / fx * 2.5, 0.02)
    ys = np.arange(-(H / 2 + 2) / fx * 2.5, (H / 2 + 2) / fx * 2.5, 0.02)
    gx, gy = np.meshgrid(xs, ys)
    cam = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, sign * 2.5), np.ones(gx.size)], 1)
    env = (cam @ c2w.T)[:, :3]
    return dict(H=H, W=W, kind=kind, z_forward=z_forward, seed=seed, depth=depth.astype(F), inv_K=inv_K.astype(F), c2w=c2w.astype(F),
                env=env.astype(F))


def depth_kinv(c):
    """float32 [3,3], as the drop-in and the reference take it on the host"""
    import torch
    from fisher_rast.cloud import novelty_kinv
    return novelty_kinv(torch.from_numpy(c["inv_K"])).numpy()


def np_depth_points(c, stride, dtype=np.float64):
    """the reference's chain in NumPy: (points [Hs,Ws,3], valid [Hs,Ws])"""
    H, W = c["H"], c["W"]
    vv, uu = np.meshgrid(np.arange(0, H, stride), np.arange(0, W, stride), indexing="ij")
    d = c["depth"][vv, uu].astype(dtype)
    valid = np.isfinite(d) & (d > 0)
    kinv = depth_kinv(c).astype(dtype)
    rays = np.einsum("ij,hwj->hwi", kinv, np.stack([uu, vv, np.ones_like(uu)], -1).astype(dtype))
    with np.errstate(invalid="ignore", over="ignore"):
        pc = rays * d[..., None]
        if c["z_forward"] in ("-Z", "-z"):
            pc[..., 2] *= -1
        pw = np.einsum("ij,hwj->hwi", c["c2w"][:3, :3].astype(dtype), pc) + c["c2w"][:3, 3].astype(dtype)
    return pw, valid


def qualifies_depth(c, stride, dist_th=0.05):
    pw, valid = np_depth_points(c, stride)
    if not valid.any():
        return True
    d = scipy_nearest(c["env"], pw[valid])[0]
    return bool(np.abs(c["env"]).max() < COORD_LIMIT and np.abs(pw[valid]).max() < COORD_LIMIT and not (np.abs(d - dist_th) <= DEPTH_MARGIN).any())


def qualifying_depth_case(H, W, kind, z_forward, strides=(1, 2, 3)):
    for seed in range(MAX_SEEDS):
        c = make_depth_case(H, W, kind, z_forward, seed)
        if all(qualifies_depth(c, s) for s in strides):
            return c
    raise AssertionError(f"no qualifying seed for depth {H}x{W} {kind} {z_forward}")


def scipy_novelty_mask(c, stride, dist_th=0.05):
    """novelty_mask_from_pcd_nn from the float64 statement"""
    pw, valid = np_depth_points(c, stride)
    if not valid.any():
        return np.zeros((c["H"], c["W"]), np.uint8)
    mask = np.zeros(valid.shape, np.uint8)
    mask[valid] = scipy_nearest(c["env"], pw[valid])[0] > dist_th
    return mask if (mask > 0).sum() >= 20 else np.zeros((c["H"], c["W"]), np.uint8)


# ---- the golden cases (tests/golden/make_reference_cloud_vectors.py runs the reference's functions on them) ---------------------------

GOLDEN_POINTS = (("uniform", 1025, 257), ("clusters", 2049, 1000), ("surface", 5000, 1000), ("outside", 1023, 65))
GOLDEN_DEPTH = ((48, 64, "object", "-Z", 1), (47, 63, "object", "Z", 2), (47, 63, "object", "-z", 3), (48, 64, "few", "-Z", 2),
                (48, 64, "none-valid", "Z", 2))


# ---- the harness ----------------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_cloud_harness"))
    vp = ctypes.c_void_p
    h.frc_h_dist2.argtypes = [vp, vp]
    h.frc_h_dist2.restype = ctypes.c_float
    h.frc_h_box_dist2.argtypes = [vp, vp, vp]
    h.frc_h_box_dist2.restype = ctypes.c_float
    h.frc_h_morton.argtypes = [vp, vp, vp]
    h.frc_h_morton.restype = ctypes.c_uint32
    h.frc_h_depth_points.argtypes = [ctypes.c_int] * 4 + [vp] * 5
    h.frc_h_depth_points.restype = None
    h.frc_h_query.argtypes = [ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.c_int, ctypes.c_float] + [vp] * 4
    h.frc_h_query.restype = None
    return h


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def decode(stats):
    """the four 8-byte words as dict(sum, valid, flagged, skipped)"""
    w = np.ascontiguousarray(stats).view(np.int64).reshape(-1)
    return dict(sum=float(w[:1].view(np.float64)[0]), valid=int(w[1]), flagged=int(w[2]), skipped=int(w[3]))


def harness_query(h, targets, queries, dist_th, valid=None, novel=False):
    """dict(dist float32 [M], idx int32 [M], flag uint8 [M], stats uint64 [4])"""
    t, q = np.ascontiguousarray(targets, F).reshape(-1, 3), np.ascontiguousarray(queries, F).reshape(-1, 3)
    M = q.shape[0]
    out = dict(dist=np.empty(M, F), idx=np.empty(M, np.int32), flag=np.empty(M, np.uint8), stats=np.zeros(4, np.uint64))
    v = None if valid is None else np.ascontiguousarray(valid, np.uint8).reshape(-1)
    h.frc_h_query(t.shape[0], _p(t), M, _p(q), _p(v), int(novel), float(dist_th), _p(out["dist"]), _p(out["idx"]), _p(out["flag"]), _p(out["stats"]))
    return out


def harness_depth(h, c, stride, dist_th=0.05):
    """the depth mode: dict(points [Hs,Ws,3], valid, dist, idx, flag (each [Hs,Ws]), stats)"""
    H, W = c["H"], c["W"]
    Hs, Ws = (H + stride - 1) // stride, (W + stride - 1) // stride
    kinv = np.ascontiguousarray(depth_kinv(c), F)
    c2w = np.ascontiguousarray(c["c2w"][:3, :4], F)
    depth = np.ascontiguousarray(c["depth"], F)
    pts, valid = np.empty((Hs * Ws, 3), F), np.empty(Hs * Ws, np.uint8)
    h.frc_h_depth_points(H, W, stride, int(c["z_forward"] in ("-Z", "-z")), _p(depth), _p(kinv), _p(c2w), _p(pts), _p(valid))
    r = harness_query(h, c["env"], pts, dist_th, valid=valid, novel=True)
    return dict(points=pts.reshape(Hs, Ws, 3), valid=valid.reshape(Hs, Ws), dist=r["dist"].reshape(Hs, Ws), idx=r["idx"].reshape(Hs, Ws),
                flag=r["flag"].reshape(Hs, Ws), stats=r["stats"])


def harness_metrics(h, gt, rec, dist_th):
    """accuracy_comp_ratio_from_pcl and reconstruction_metrics over the harness: the product's host arithmetic on the harness's statistics"""
    from fisher_rast.cloud import metrics_from_stats
    return metrics_from_stats(decode(harness_query(h, gt, rec, dist_th)["stats"]), decode(harness_query(h, rec, gt, dist_th)["stats"]))


def harness_novelty_mask(h, c, stride, dist_th=0.05):
    """novelty_mask_from_pcd_nn over the harness"""
    from fisher_rast.cloud import novelty_mask_from_host
    r = harness_depth(h, c, stride, dist_th)
    return novelty_mask_from_host(r["flag"].copy(), decode(r["stats"]), c["H"], c["W"])
