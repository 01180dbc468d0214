"""Inputs, a NumPy restatement and a reference-order torch chain for the keyframe overlap (fr_keyframe_valid_pixels /
fr_keyframe_overlap, models/SLAM/utils/keyframe_selection.py).

The cases are regenerated from seeds, not stored.  `np_overlap` restates csrc/fr_keyframe_math.h (over fr_ingest_math.h) with the
headers' operand order in a dtype of the caller's choice: in binary32 every operation is one of + - x / rint, each correctly rounded
in NumPy as in the header, so it reproduces the g++ harness bit for bit; in binary64 it is the yardstick by which a case
*qualifies* for a comparison with torch, whose matmul does not promise our summation order (see `qualifies`).  `torch_chain` is the
reference's chain (torch.where, unique / isin, torch.inverse, matmul per keyframe, a sort of 0-dim tensors) in this helper's own
form, on any device.  The g++ harness (tests/harness/fr_keyframe_harness.cpp) is bound here too, also as a backend of the product's
KeyframeSelection, which has no CPU path of its own."""

import numpy as np

import cameras
import harness_build

# qualifying families may be compared with torch and the golden file once `qualifies` holds; the adversarial ones sit on the
# decisions themselves (equal keys, thresholds) and are compared with the harness / the binary32 restatement only
QUALIFYING = ["generic", "masks-present", "masks-mixed", "behind", "curr-mask"]
ADVERSARIAL = ["wall", "dup-draws", "all-invalid", "zero-depth-in-mask", "edges", "curr-mask-empty", "masks-absent-edge0"]
FAMILIES = QUALIFYING + ADVERSARIAL
MAX_SEEDS = 8
# margins of a qualifying case, in binary64: about 40 times the binary32 evaluation error for coordinates below 512 px and 10 m
# (2.5e-4 px, 1e-5 m)
MARGIN_PX, MARGIN_Z, MARGIN_M = 1e-2, 1e-4, 1e-3


def rigid(yaw=0.0, pitch=0.0, t=(0.0, 0.0, 0.0)):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m = np.eye(4)
    m[:3, :3] = Ry @ Rx
    m[:3, 3] = t
    return m


def make_case(family, seed=0, H=48, W=64, n=None, K=None):
    """dict(H, W, K [3,3], w2c [4,4], depth [1,H,W], curr_mask [H,W] bool or None, valid_idx int32, draws int64 [n], kf_w2c [K,4,4],
    kf_masks (list of [H,W] bool or None), edge), float32.  The draws are torch.randint's under torch.manual_seed(seed), as the
    product draws them."""
    import torch
    rng = np.random.default_rng([FAMILIES.index(family), seed, H, W, 20250607])
    edge = 4
    n = n if n is not None else (16 if family.startswith("masks") else 48)
    nk = K if K is not None else 4
    intr = np.array([[0.9 * W, 0, 0.47 * W], [0, 1.1 * H, 0.55 * H], [0, 0, 1]], np.float32)
    w2c = np.ascontiguousarray(cameras.pose(), np.float32)
    depth = rng.uniform(0.8, 4.0, (H, W)).astype(np.float32)
    depth[rng.uniform(size=(H, W)) < 0.05] = 0.0
    curr_mask = None
    poses = [rigid(rng.uniform(-0.25, 0.25), rng.uniform(-0.15, 0.15), rng.uniform(-0.4, 0.4, 3)) for _ in range(nk)]
    kf_masks = [None] * nk
    draws = None
    if family == "generic":
        pass
    elif family in ("masks-present", "masks-mixed"):
        for k in range(nk):
            if family == "masks-present" or k % 2 == 0:
                coarse = rng.uniform(size=((H + 7) // 8, (W + 7) // 8)) < 0.6                 # 8 x 8 blocks
                kf_masks[k] = coarse[np.arange(H)[:, None] // 8, np.arange(W)[None, :] // 8]
    elif family == "behind":
        for k in range(0, nk, 2):
            poses[k] = rigid(np.pi + rng.uniform(-0.1, 0.1), 0.0, rng.uniform(-0.2, 0.2, 3))          # looks the other way
    elif family == "curr-mask":
        curr_mask = rng.uniform(size=(H, W)) < 0.3
    elif family == "curr-mask-empty":
        curr_mask = np.zeros((H, W), bool)
    elif family == "wall":
        # a flat wall seen head-on through a centred camera at the world origin: pixels left and right of the centre column give
        # (x, y, z) and (-x, y, z), which the reference's filter takes for one point
        intr = np.array([[32, 0, W // 2], [0, 32, H // 2], [0, 0, 1]], np.float32)
        w2c = np.eye(4, dtype=np.float32)
        depth[:] = 2.0
        poses = [rigid(0.0, 0.0, (0.0, 0.0, 0.1 * k)) for k in range(nk)]
    elif family == "dup-draws":
        pass
    elif family == "all-invalid":
        pass
    elif family == "zero-depth-in-mask":
        curr_mask = np.zeros((H, W), bool)
        curr_mask[10:20, 10:30] = True
        depth[10:20, 10:30] = rng.uniform(1.0, 2.0, (10, 20)).astype(np.float32)
        depth[12, 15] = 0.0                                                   # inside the mask, without a depth
        depth[19, 29] = 0.0
    elif family in ("edges", "masks-absent-edge0"):
        # identity poses, power-of-two focal lengths, integer principal point and a depth of 256: every operation is exact, and
        # 256 + 1e-5 rounds to 256, so u == x and v == y -- the pixels on the four thresholds project exactly onto them
        intr = np.array([[32, 0, W // 2 + 3], [0, 64, H // 2 - 2], [0, 0, 1]], np.float32)
        w2c = np.eye(4, dtype=np.float32)
        depth[:] = 256.0
        poses = [np.eye(4) for _ in range(nk)]
        edge = 2 if family == "edges" else 0
    else:
        raise ValueError(family)
    ok = depth > 0
    if curr_mask is not None:
        ok &= curr_mask
    valid_idx = np.flatnonzero(ok.reshape(-1)).astype(np.int32)
    count = int(valid_idx.size)
    torch.manual_seed(seed)
    if count:
        draws = torch.randint(count, (min(n, count),)).numpy().astype(np.int64)
    else:
        draws = np.zeros(0, np.int64)
    if family == "dup-draws" and count:
        draws[1::3] = draws[0::3][:len(draws[1::3])]                          # every third draw repeats its neighbour
    elif family == "all-invalid" and count:
        half = draws[:len(draws) // 2]
        draws = np.concatenate([half, half])                                  # every pixel drawn twice: nothing survives
    elif family in ("edges", "masks-absent-edge0") and count:
        e = edge
        on = [(e, 10), (W - e, 11), (13, e), (14, H - e), (e + 1, 12), (W - e - 1, 15), (16, e + 1), (17, H - e - 1), (e, e), (W - e, H - e)]
        on = [(min(x, W - 1), min(y, H - 1)) for x, y in on]
        draws[:len(on)] = [int(np.searchsorted(valid_idx, y * W + x)) for x, y in on]
    kf = np.stack([(p @ w2c.astype(np.float64)) for p in poses]).astype(np.float32) if nk else np.zeros((0, 4, 4), np.float32)
    return dict(H=H, W=W, K=intr, w2c=w2c, depth=depth[None].copy(), curr_mask=curr_mask, valid_idx=valid_idx, draws=draws,
                kf_w2c=np.ascontiguousarray(kf), kf_masks=kf_masks, edge=edge, family=family, seed=seed)


# ---- the restatement of csrc/fr_keyframe_math.h in a dtype of the caller's choice -------------------------------------------------

def np_invert_affine(w2c, F):
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


def np_valid_pixels(c):
    ok = c["depth"][0] > 0
    if c["curr_mask"] is not None:
        ok = ok & (np.asarray(c["curr_mask"]) != 0)
    return np.flatnonzero(ok.reshape(-1)).astype(np.int32)


def np_overlap(c, F=np.float32, valid_idx="case", draws=None, edge=None):
    """dict(pts [n,3], keys, valid [n] bool, oor [n] bool, counts [K], uv [K,n,2], z [K,n], inside [K,n], n_valid, n_oor, pix [n]) in
    dtype F.  valid_idx: "case" (the case's list), None (a draw is a pixel) or an int32 array."""
    H, W = c["H"], c["W"]
    edge = c["edge"] if edge is None else edge
    vi = c["valid_idx"] if isinstance(valid_idx, str) else valid_idx
    d = np.asarray(c["draws"] if draws is None else draws, np.int64)
    limit = H * W if vi is None else len(vi)
    in_draw = (d >= 0) & (d < limit)
    pix = np.full(d.shape, -1, np.int64)
    pix[in_draw] = d[in_draw] if vi is None else np.asarray(vi, np.int64)[d[in_draw]]
    oor = ~((pix >= 0) & (pix < H * W))
    p = np.where(oor, 0, pix)
    x, y = p % W, p // W
    intr, m = c["K"].astype(F), np_invert_affine(c["w2c"], F)
    fx, fy, cx, cy = intr[0, 0], intr[1, 1], intr[0, 2], intr[1, 2]
    z = c["depth"].reshape(-1)[p].astype(F)
    xx, yy = (x.astype(F) - cx) / fx, (y.astype(F) - cy) / fy
    X, Y = xx * z, yy * z
    pts = np.stack([((m[r, 0] * X + m[r, 1] * Y) + m[r, 2] * z) + m[r, 3] for r in range(3)], 1).astype(F)
    pts[oor] = 0
    keys = np.abs(np.rint(pts * F(1e4)) / F(1e4)).astype(F)
    same = (keys[:, None, :] == keys[None, :, :]).all(-1) & ~oor[None, :]
    np.fill_diagonal(same, False)
    valid = ~(same.any(1) | (keys == 0).all(1) | oor)
    nk = c["kf_w2c"].shape[0]
    n = len(d)
    uv, zz, inside, counts = np.zeros((nk, n, 2), F), np.zeros((nk, n), F), np.zeros((nk, n), bool), np.zeros(nk, np.int32)
    for k in range(nk):
        w = c["kf_w2c"][k].astype(F)
        cam = [((w[r, 0] * pts[:, 0] + w[r, 1] * pts[:, 1]) + w[r, 2] * pts[:, 2]) + w[r, 3] for r in range(3)]
        q = [(intr[r, 0] * cam[0] + intr[r, 1] * cam[1]) + intr[r, 2] * cam[2] for r in range(3)]
        zk = q[2] + F(np.float32(1e-5))
        with np.errstate(divide="ignore", invalid="ignore"):
            u, v = q[0] / zk, q[1] / zk
        ins = (u < F(W - edge)) & (u > F(edge)) & (v < F(H - edge)) & (v > F(edge)) & (zk > 0)
        mk = c["kf_masks"][k]
        if mk is not None:
            with np.errstate(invalid="ignore"):
                iu = np.clip(np.rint(np.where(ins, u, 0)), 0, W - 1).astype(np.int64)
                iv = np.clip(np.rint(np.where(ins, v, 0)), 0, H - 1).astype(np.int64)
            ins = ins & (np.asarray(mk)[iv, iu] != 0)
        ins = ins & valid
        uv[k, :, 0], uv[k, :, 1], zz[k], inside[k], counts[k] = u, v, zk, ins, int(ins.sum())
    return dict(pts=pts, keys=keys, valid=valid, oor=oor, counts=counts, uv=uv, z=zz, inside=inside, n_valid=int(valid.sum()),
                n_oor=int(oor.sum()), pix=pix)


def qualifies(c):
    """whether every decision of the case is clear of its threshold in binary64 by the margins above, so that any binary32
    evaluation -- ours or torch's, whatever its summation order -- decides alike"""
    r = np_overlap(c, np.float64)
    H, W, e = c["H"], c["W"], c["edge"]
    if r["n_oor"] or len(c["draws"]) == 0:
        return False
    p, pix = np.abs(r["pts"]), r["pix"]
    if (np.linalg.norm(r["pts"], axis=1) < MARGIN_M).any():
        return False
    distinct = pix[:, None] != pix[None, :]
    close = (np.abs(p[:, None, :] - p[None, :, :]).max(-1) <= MARGIN_M) & distinct
    if close.any():
        return False
    v = r["valid"]
    for k in range(c["kf_w2c"].shape[0]):
        u, w, z = r["uv"][k, v, 0], r["uv"][k, v, 1], r["z"][k, v]
        if (np.abs(z) < MARGIN_Z).any():
            return False
        for val, lim in ((u, W), (w, H)):
            if (np.abs(val - (lim - e)) < MARGIN_PX).any() or (np.abs(val - e) < MARGIN_PX).any():
                return False
        if c["kf_masks"][k] is not None:
            ins = (u < W - e) & (u > e) & (w < H - e) & (w > e) & (z > 0)         # the mask is read for these only
            for val in (u[ins], w[ins]):
                if (np.abs(np.abs(val - np.floor(val)) - 0.5) < MARGIN_PX).any():
                    return False
    return True


def qualifying_case(family, H=48, W=64, **kw):
    """the first of MAX_SEEDS seeds at which the family's case qualifies"""
    for seed in range(MAX_SEEDS):
        c = make_case(family, seed, H, W, **kw)
        if qualifies(c):
            return c
    raise AssertionError(f"{family}: no qualifying case within {MAX_SEEDS} seeds")


def keyframe_list(c, dev="cpu", mask_key="obj_mask_2d"):
    import torch
    out = []
    for k in range(c["kf_w2c"].shape[0]):
        kf = {"est_w2c": torch.from_numpy(c["kf_w2c"][k].copy()).to(dev)}
        if c["kf_masks"][k] is not None:
            kf[mask_key if k % 4 else "mask"] = torch.from_numpy(np.ascontiguousarray(c["kf_masks"][k])).to(dev)
        out.append(kf)
    return out


# ---- the reference-order chain in torch ------------------------------------------------------------------------------------------

def torch_pointcloud(depth, intrinsics, w2c, rowcol, record=None):
    """the kept world points [M,3] of the pixels rowcol [n,2], as keyframe_selection.py:10-37 forms them"""
    import torch
    fx, fy, cx, cy = intrinsics[0][0], intrinsics[1][1], intrinsics[0][2], intrinsics[1][2]
    z = depth[0, rowcol[:, 0], rowcol[:, 1]]
    cam = torch.stack(((rowcol[:, 1] - cx) / fx * z, (rowcol[:, 0] - cy) / fy * z, z), dim=-1)
    cam4 = torch.cat([cam, torch.ones_like(cam[:, :1])], dim=1).float()
    pts = (torch.inverse(w2c) @ cam4.T).T[:, :3]
    keys = torch.abs(torch.round(pts, decimals=4))
    zero = torch.zeros((1, 3), device=pts.device, dtype=torch.float32)
    _, inverse, counts = torch.cat([keys, zero], dim=0).unique(dim=0, return_inverse=True, return_counts=True)
    repeated = torch.isin(inverse, torch.where(counts.gt(1))[0])[:len(keys)]
    if record is not None:
        record["pts_all"], record["valid"] = pts, ~repeated
    return pts[~repeated]


def torch_chain(gt_depth, w2c, intrinsics, keyframes, k, curr_mask=None, pixels=1600, edge=20, record=None):
    """keyframe_selection_overlap as keyframe_selection.py:40-134 computes it: same draws from the CPU generator, one small chain
    per keyframe, a sort of 0-dim tensors, np.random.permutation; tensors on any device.  `record` receives pts, percent, draws."""
    import torch
    import torch.nn.functional as Fn
    H, W = gt_depth.shape[1], gt_depth.shape[2]
    ok = gt_depth[0] > 0
    if curr_mask is not None:
        ok = ok & curr_mask.bool()
    rowcol = torch.stack(torch.where(ok), dim=1)
    if rowcol.shape[0] == 0:
        return []
    draws = torch.randint(rowcol.shape[0], (min(pixels, rowcol.shape[0]),))
    pts = torch_pointcloud(gt_depth, intrinsics, w2c, rowcol[draws], record)
    entries = []
    for i, kf in enumerate(keyframes):
        pts4 = torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)
        cam = (kf["est_w2c"] @ pts4.T).T[:, :3]
        q = torch.matmul(intrinsics, cam.transpose(0, 1)).transpose(0, 1)
        z = q[:, 2:] + 1e-5
        uv = (q / z)[:, :2]
        ins = (uv[:, 0] < W - edge) * (uv[:, 0] > edge) * (uv[:, 1] < H - edge) * (uv[:, 1] > edge)
        ins = ins & (z[:, 0] > 0)
        m = kf.get("obj_mask_2d", None)
        if m is None:
            m = kf.get("mask", None)
        if m is not None:
            m = m.bool()
            if m.shape[-2:] != (H, W):
                m = Fn.interpolate(m[None, None].float(), size=(H, W), mode="nearest")[0, 0].bool()
            iu = uv[:, 0].round().long().clamp(0, W - 1)
            iv = uv[:, 1].round().long().clamp(0, H - 1)
            ins = ins & m[iv, iu]
        entries.append((i, ins.sum() / uv.shape[0]))
    if record is not None:
        record["pts"], record["draws"] = pts, draws
        record["percent"] = [float(p) for _, p in entries]
    entries = sorted(entries, key=lambda e: e[1], reverse=True)
    chosen = [i for i, p in entries if p > 0.0]
    return list(np.random.permutation(np.array(chosen))[:k])


# ---- the g++ harness (tests/harness/fr_keyframe_harness.cpp) ---------------------------------------------------------------------

def build_harness():
    import ctypes
    h = ctypes.CDLL(harness_build.shared("fr_keyframe_harness"))
    vp = ctypes.c_void_p
    h.frk_valid_pixels.argtypes = [ctypes.c_int, ctypes.c_int, vp, vp, vp, vp]
    h.frk_valid_pixels.restype = None
    h.frk_key_of.argtypes = [ctypes.c_float]
    h.frk_key_of.restype = ctypes.c_float
    h.frk_overlap.argtypes = [ctypes.c_int] * 6 + [vp] * 12
    h.frk_overlap.restype = None
    return h


def _ptr(a):
    return None if a is None else a.ctypes.data


def harness_valid_pixels(h, depth, mask=None):
    """(idx int32 [count], status [4])"""
    d = np.ascontiguousarray(depth, np.float32)
    H, W = d.shape[-2], d.shape[-1]
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
    idx, status = np.zeros(H * W, np.int32), np.zeros(4, np.int32)
    h.frk_valid_pixels(H, W, _ptr(d), _ptr(m), _ptr(idx), _ptr(status))
    return idx[:int(status[0])].copy(), status


def harness_overlap(h, c, valid_idx="case", draws=None, edge=None, kf_masks="case"):
    """dict(counts [K], valid [n] uint8, pts [n,3], status [4], uv [K,n,2])"""
    H, W = c["H"], c["W"]
    vi = c["valid_idx"] if isinstance(valid_idx, str) else valid_idx
    vi = None if vi is None else np.ascontiguousarray(vi, np.int32)
    d = np.ascontiguousarray(c["draws"] if draws is None else draws, np.int64)
    masks = c["kf_masks"] if isinstance(kf_masks, str) else kf_masks
    kf = np.ascontiguousarray(c["kf_w2c"], np.float32)
    nk, n = kf.shape[0], len(d)
    keep = [None if m is None else np.ascontiguousarray(np.asarray(m) != 0, np.uint8) for m in (masks or [])]
    table = np.array([0 if m is None else m.ctypes.data for m in keep], np.uint64) if any(m is not None for m in keep) else None
    out = dict(counts=np.zeros(nk, np.int32), valid=np.zeros(n, np.uint8), pts=np.zeros((n, 3), np.float32), status=np.zeros(4, np.int32),
               uv=np.zeros((nk, n, 2), np.float32))
    depth = np.ascontiguousarray(c["depth"], np.float32)
    h.frk_overlap(H, W, n, nk, c["edge"] if edge is None else edge, 0 if vi is None else len(vi), _ptr(np.ascontiguousarray(c["K"], np.float32)),
                  _ptr(np.ascontiguousarray(c["w2c"], np.float32)), _ptr(depth), _ptr(vi), _ptr(d), _ptr(kf), _ptr(table),
                  *(_ptr(out[k]) for k in ("counts", "valid", "pts", "status", "uv")))
    return out


class HarnessBackend:
    """the two calls of models/SLAM/utils/keyframe_selection.py's backend on host tensors, through the g++ harness: the product's
    host logic (draws, masks, the two reads, the sort and the permutation) runs on the CPU over the kernels' own arithmetic"""

    def __init__(self, h):
        self.h = h
        self.calls = []

    def valid_pixels(self, depth, mask=None):
        import torch
        idx, status = harness_valid_pixels(self.h, depth.numpy(), None if mask is None else mask.numpy())
        full = np.zeros(depth.numel(), np.int32)
        full[:len(idx)] = idx
        self.calls.append("valid_pixels")
        return torch.from_numpy(full), torch.from_numpy(status.copy())

    def overlap(self, depth, intrinsics, w2c, draws, kf_w2c, *, valid_idx=None, n_valid_idx=None, kf_masks=None, edge=20, want_valid=True,
                want_pts=False):
        import torch
        H, W = int(depth.shape[-2]), int(depth.shape[-1])
        vi = None if valid_idx is None else valid_idx.numpy()[:valid_idx.numel() if n_valid_idx is None else n_valid_idx]
        c = dict(H=H, W=W, K=np.asarray(intrinsics, np.float32)[:3, :3], w2c=np.asarray(w2c, np.float32), depth=depth.numpy(),
                 kf_w2c=np.asarray(kf_w2c, np.float32).reshape(-1, 4, 4), edge=edge,
                 kf_masks=None if kf_masks is None else [None if m is None else m.numpy() for m in kf_masks])
        out = harness_overlap(self.h, c, valid_idx=vi, draws=np.asarray(draws, np.int64), kf_masks=c["kf_masks"])
        self.calls.append("overlap")
        return dict(counts=torch.from_numpy(out["counts"]), status=torch.from_numpy(out["status"]),
                    valid=torch.from_numpy(out["valid"]) if want_valid else None, pts=torch.from_numpy(out["pts"]) if want_pts else None)
