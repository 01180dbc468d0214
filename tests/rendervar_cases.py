"""Inputs, the torch restatement of the chain (binary64 and binary32), the stage rules against binary64 and a CPU backend for the
fused render-variable build (fr_rendervar_forward / fr_rendervar_backward, csrc/fr_rendervar.hip; fisher_rast/rendervar.py).

`torch_chain` restates, from their description, the ops between `params` and the rasteriser of the reference's training step --
F.normalize of the camera quaternion, build_rotation (which normalises again), eye(4) with two slice assignments, ones / cat / matmul
for the points, cat / matmul / square for the (z, 1, z^2) features, F.normalize / sigmoid / tile + exp for the activations -- and
autograd differentiates it.  `stages` evaluates every stage of the kernels' arithmetic (csrc/fr_rendervar_math.h) in binary64 on
that stage's binary32 inputs, with the sum of the magnitudes of its terms; `HarnessBackend` is the CPU stand-in for
rendervar.HipRenderVarBackend, the g++ build of the header (tests/harness/fr_rendervar_harness.cpp) on CPU tensors."""
import ctypes

import numpy as np
import torch
import torch.nn.functional as tF
import harness_build

F = np.float32
EPS_N = 1e-12
T_FRAMES = 5

# Each stage against the binary64 evaluation of the same stage on the same binary32 inputs: |got - want64| <= K 2^-24 sum|terms| +
# 2^-149.  K needed by torch's own float32 chain on the CPU, stage by stage, over P = 1, 65, 1000, both scale layouts and three frames
# on one thread (printed by tests/test_rendervar_cpu.py, which fails when a measurement exceeds the figure recorded here; DESIGN.md
# section 2 has them too); the kernels' arithmetic is allowed twice that, under the project's cap of 16.
K_TORCH_CPU = {
    "pose": 2.91, "pts": 2.46, "feats": 2.32, "rotations": 2.64, "opacities": 1.78, "scales": 0.99,
    "G": 3.06, "g_means3D": 2.0, "g_unnorm_rotations": 5.7, "g_logit_opacities": 2.35, "g_log_scales": 2.03, "tail": 3.23,
}
# The twelve sums over P, dR = sum G (x) m and dt = sum G: the K that torch's float32 matmul backward needs at the P of a test (the sum
# of |terms| grows with P, the error of a blocked sum like its root, so the figure falls as P grows) -- the largest over the seeds of
# `torch_sums_need`, on one thread.  1000 and below are the CPU suite's sizes; the others are the GPU suite's (around a wave, around
# a workgroup of 256 rows, and a capped grid of 2048 workgroups plus a workgroup and a tail).
K_TORCH_SUMS_AT = {1: 0.89, 3: 1.42, 63: 1.8, 64: 2.42, 65: 2.32, 255: 1.33, 256: 1.37, 257: 2.15, 1000: 0.99, 2000: 0.65, 524549: 0.08}


def allowed(stage):
    return min(16.0, round(2 * K_TORCH_CPU[stage], 1))


def allowed_sums(P):
    return min(16.0, round(2 * K_TORCH_SUMS_AT[P], 2))


def torch_sums_need(P):
    """the K torch's float32 matmul backward needs for the twelve sums at P rows: seeds 0 .. 7 (0 .. 2 above 10 000 rows), three scale
    columns, frame 1, one thread (the blocking of a threaded matmul depends on the machine)"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        need = 0.0
        for seed in range(8 if P < 10000 else 3):
            inp = make_inputs(P, 3, seed=seed)
            need = max(need, k_need(*stages(inp, 1, torch32_staged(inp, 1))["sums"]))
        return need
    finally:
        torch.set_num_threads(threads)


def camera_bound(inp, time_idx, vals, P):
    """the bound on the seven camera gradients of an implementation that sums the twelve in binary32: the sums' allowance at P and
    the tail's, each carried through the tail -- allowed_sums(P) 2^-24 tail(sum|terms|) + allowed('tail') 2^-24 tail(|sums|).  `vals`
    holds the harness's 'G' and binary64 'sums'.  Returns (want [7], bound [7]): the harness's tail on its own sums is the yardstick."""
    d = np.float64
    G, m = np.asarray(vals["G"]).astype(d), inp["means3D"].astype(d)
    cq = inp["cam_unnorm_rots"][0, :, time_idx].astype(d)
    t_sums = np.concatenate([(np.abs(G).T @ np.abs(m)).reshape(-1), np.abs(G).sum(0)])
    sums = np.asarray(vals["sums"], d)
    want = np.concatenate(tail64(cq, sums[:9].reshape(3, 3), sums[9:]))
    from_sums = np.concatenate(tail64(cq, t_sums[:9].reshape(3, 3), t_sums[9:], magnitudes=True))
    from_tail = np.concatenate(tail64(cq, sums[:9].reshape(3, 3), sums[9:], magnitudes=True))
    from_tail[4:] = 0.0                                     # the translation's gradient is the sums themselves
    return want, 2.0 ** -24 * (allowed_sums(P) * from_sums + allowed("tail") * from_tail) + 2.0 ** -149


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits_or_both_nan(got, want):
    """bit for bit, except that a NaN matches any NaN: default-NaN payloads differ between hosts"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


# ---- inputs ----------------------------------------------------------------------------------------------------------------------

def random_rigid(rng):
    q = rng.normal(size=4)
    r, x, y, z = q / np.linalg.norm(q)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                  [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                  [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, rng.normal(size=3)
    return m


def make_inputs(P, scale_cols, seed=0, identity_w2c=False, frames=T_FRAMES):
    """float32 arrays: the four per-Gaussian parameters, the camera arrays [1,4,T] / [1,3,T], first_frame_w2c and the five upstream
    gradients, at the scales the issue sets"""
    rng = np.random.default_rng([seed, P, scale_cols])
    d = {
        "means3D": 4 * rng.normal(size=(P, 3)),
        "unnorm_rotations": rng.normal(size=(P, 4)),
        "logit_opacities": 3 * rng.normal(size=(P, 1)),
        "log_scales": rng.normal(size=(P, scale_cols)) - 3,
        "cam_unnorm_rots": 0.7 * rng.normal(size=(1, 4, frames)),
        "cam_trans": rng.normal(size=(1, 3, frames)),
        "first_frame_w2c": np.eye(4) if identity_w2c else random_rigid(rng),
        "g_pts": rng.normal(size=(P, 3)), "g_feats": rng.normal(size=(P, 3)), "g_rotations": rng.normal(size=(P, 4)),
        "g_opacities": rng.normal(size=(P, 1)), "g_scales": rng.normal(size=(P, 3)),
    }
    return {k: np.ascontiguousarray(v, F) for k, v in d.items()}


PARAMS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")
OUTPUTS = ("pts", "feats", "rotations", "opacities", "scales")
UPSTREAM = ("g_pts", "g_feats", "g_rotations", "g_opacities", "g_scales")
GRADS = ("g_means3D", "g_unnorm_rotations", "g_logit_opacities", "g_log_scales", "g_cam_unnorm_rots", "g_cam_trans")


# ---- the torch restatement of the chain --------------------------------------------------------------------------------------------

def t_rotation(quat):
    """[N,3,3] rotation matrices of the quaternions [N,4] (w first), with the op structure of the chain under test: the argument is
    normalised here once more, by the root of its four squared components added left to right, and the nine entries are written one
    at a time into a zero matrix"""
    w, x, y, z = quat.unbind(dim=1)
    length = torch.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = (quat / length.unsqueeze(1)).unbind(dim=1)
    entries = {
        (0, 0): lambda: 1 - 2 * (y * y + z * z), (0, 1): lambda: 2 * (x * y - w * z), (0, 2): lambda: 2 * (x * z + w * y),
        (1, 0): lambda: 2 * (x * y + w * z), (1, 1): lambda: 1 - 2 * (x * x + z * z), (1, 2): lambda: 2 * (y * z - w * x),
        (2, 0): lambda: 2 * (x * z - w * y), (2, 1): lambda: 2 * (y * z + w * x), (2, 2): lambda: 1 - 2 * (x * x + y * y),
    }
    out = quat.new_zeros((quat.shape[0], 3, 3))
    for (i, j), value in entries.items():
        out[:, i, j] = value()
    return out


def t_pose(cq, ct):
    """[4,4] rel_w2c from the frame's quaternion [1,4] and translation [1,3]"""
    rel = torch.eye(4, dtype=cq.dtype, device=cq.device)
    rel[:3, :3] = t_rotation(tF.normalize(cq))
    rel[:3, 3] = ct
    return rel


def t_points(rel, means):
    pts4 = torch.cat((means, torch.ones_like(means[:, :1])), dim=1)
    return (rel @ pts4.T).T[:, :3]


def t_feats(w2c, pts):
    pts4 = torch.cat((pts, torch.ones_like(pts[:, :1])), dim=-1)
    z = (w2c @ pts4.transpose(0, 1)).transpose(0, 1)[:, 2:3]
    return torch.cat((z, torch.ones_like(z), torch.square(z)), dim=1)


def t_scales(ls):
    return torch.exp(ls if ls.shape[-1] == 3 else torch.tile(ls, (1, 3)))


def torch_chain(inp, time_idx, gaussians_grad, camera_grad, dtype=torch.float64, device="cpu"):
    """{output or gradient name: tensor of `dtype`}: the whole chain forward, then autograd with the upstream gradients of `inp`.
    Gradients follow transform_to_frame's flags: means3D only with gaussians_grad, the camera arrays only with camera_grad (None
    otherwise)."""
    t = {k: torch.from_numpy(v).to(device=device, dtype=dtype) for k, v in inp.items()}
    p = {k: t[k].clone().requires_grad_(True) for k in PARAMS}
    cq, ct = p["cam_unnorm_rots"][..., time_idx], p["cam_trans"][..., time_idx]
    if not camera_grad:
        cq, ct = cq.detach(), ct.detach()
    rel = t_pose(cq, ct)
    pts = t_points(rel, p["means3D"] if gaussians_grad else p["means3D"].detach())
    out = {"rel_w2c": rel.detach(), "pts": pts, "feats": t_feats(t["first_frame_w2c"], pts), "rotations": tF.normalize(p["unnorm_rotations"]),
           "opacities": torch.sigmoid(p["logit_opacities"]), "scales": t_scales(p["log_scales"])}
    scalar = sum((out[o] * t[g]).sum() for o, g in zip(OUTPUTS, UPSTREAM) if out[o].requires_grad)
    grads = torch.autograd.grad(scalar, [p[k] for k in PARAMS], allow_unused=True)
    out = {k: v.detach() for k, v in out.items()}
    out.update({"g_" + k: g for k, g in zip(PARAMS, grads)})
    return out


# ---- the stage rules against binary64 -----------------------------------------------------------------------------------------------

def _pose64(cq):
    n1 = np.sqrt((cq * cq).sum())
    a = cq / max(n1, EPS_N)
    n2 = np.sqrt((a * a).sum())
    q = a / n2
    r, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
                  [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
                  [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]])
    TR = np.array([[1 + 2 * (y * y + z * z), 2 * (abs(x * y) + abs(r * z)), 2 * (abs(x * z) + abs(r * y))],
                   [2 * (abs(x * y) + abs(r * z)), 1 + 2 * (x * x + z * z), 2 * (abs(y * z) + abs(r * x))],
                   [2 * (abs(x * z) + abs(r * y)), 2 * (abs(y * z) + abs(r * x)), 1 + 2 * (x * x + y * y)]])
    return n1, a, n2, q, R, TR


def tail64(cq, dR, dt, magnitudes=False):
    """The pose's way back in binary64: (g_cq [4], g_ct [3]) from dR [3,3], dt [3].  With `magnitudes`, every product and sum is taken
    over absolute values instead: the sum of the magnitudes of the terms that enter each output."""
    n1, a, n2, q, _, _ = _pose64(np.asarray(cq, np.float64))
    m = (lambda v: np.abs(v)) if magnitudes else (lambda v: v)
    s = 1.0 if magnitudes else -1.0             # a difference becomes a sum of magnitudes
    r, x, y, z = m(q)
    D = m(np.asarray(dR, np.float64))
    dq = np.array([
        2 * (x * (D[2, 1] + s * D[1, 2]) + y * (D[0, 2] + s * D[2, 0]) + z * (D[1, 0] + s * D[0, 1])),
        2 * (y * (D[0, 1] + D[1, 0]) + z * (D[0, 2] + D[2, 0]) + r * (D[2, 1] + s * D[1, 2]) + s * 2 * x * (D[1, 1] + D[2, 2])),
        2 * (x * (D[0, 1] + D[1, 0]) + z * (D[1, 2] + D[2, 1]) + r * (D[0, 2] + s * D[2, 0]) + s * 2 * y * (D[0, 0] + D[2, 2])),
        2 * (x * (D[0, 2] + D[2, 0]) + y * (D[1, 2] + D[2, 1]) + r * (D[1, 0] + s * D[0, 1]) + s * 2 * z * (D[0, 0] + D[1, 1])),
    ])
    da = (dq + s * m(q) * (m(q) * dq).sum()) / n2
    g = da / EPS_N if n1 < EPS_N else (da + s * m(a) * (m(a) * da).sum()) / n1
    return g, m(np.asarray(dt, np.float64))


def stages(inp, time_idx, vals, sums_from_vals=True):
    """{stage: (got, want64, sum|terms|)} for every stage `vals` (name -> float32 array: the outputs and gradients of one
    implementation, with its 'rel_w2c', 'G' [P,3] and 'sums' [12] where it has them) can be checked at.  Each stage is evaluated in
    binary64 on the binary32 values `vals` itself fed to it."""
    d = np.float64
    x = {k: np.asarray(v, F).astype(d) for k, v in inp.items()}
    v = {k: np.asarray(a).astype(d) for k, a in vals.items() if a is not None}
    cq, ct = x["cam_unnorm_rots"][0, :, time_idx], x["cam_trans"][0, :, time_idx]
    w = x["first_frame_w2c"][2]
    out = {}
    _, _, _, _, R64, TR = _pose64(cq)
    if "rel_w2c" in v:
        out["pose"] = (v["rel_w2c"][:3, :3], R64, TR)
        R, t = v["rel_w2c"][:3, :3], v["rel_w2c"][:3, 3]
        assert np.array_equal(t, ct) and np.array_equal(v["rel_w2c"][3], [0, 0, 0, 1])
        if "pts" in v:
            out["pts"] = (v["pts"], x["means3D"] @ R.T + t, np.abs(x["means3D"]) @ np.abs(R).T + np.abs(t))
    if "feats" in v:
        zc = v["pts"] @ w[:3] + w[3]
        tz = np.abs(v["pts"]) @ np.abs(w[:3]) + abs(w[3])
        z32 = v["feats"][:, 0]
        assert np.array_equal(v["feats"][:, 1], np.ones_like(z32))
        out["feats"] = (v["feats"][:, [0, 2]], np.stack([zc, z32 * z32], 1), np.stack([tz, z32 * z32], 1))
    n = np.sqrt((x["unnorm_rotations"] ** 2).sum(1, keepdims=True))
    rot = x["unnorm_rotations"] / np.maximum(n, EPS_N)
    if "rotations" in v:
        out["rotations"] = (v["rotations"], rot, np.abs(rot))
    if "opacities" in v:
        o = 1 / (1 + np.exp(-x["logit_opacities"]))
        out["opacities"] = (v["opacities"], o, o)
    if "scales" in v:
        s = np.exp(np.broadcast_to(x["log_scales"], v["scales"].shape) if x["log_scales"].shape[1] == 1 else x["log_scales"])
        out["scales"] = (v["scales"], s, s)
    if "G" in v:
        z32 = v["feats"][:, 0:1]
        out["G"] = (v["G"], x["g_pts"] + w[:3] * (x["g_feats"][:, 0:1] + 2 * z32 * x["g_feats"][:, 2:3]),
                    np.abs(x["g_pts"]) + np.abs(w[:3]) * (np.abs(x["g_feats"][:, 0:1]) + 2 * np.abs(z32 * x["g_feats"][:, 2:3])))
        if "g_means3D" in v:
            out["g_means3D"] = (v["g_means3D"], v["G"] @ R, np.abs(v["G"]) @ np.abs(R))
        dR, tdR = v["G"].T @ x["means3D"], np.abs(v["G"]).T @ np.abs(x["means3D"])
        dt, tdt = v["G"].sum(0), np.abs(v["G"]).sum(0)
        if "sums" in v:
            out["sums"] = (v["sums"], np.concatenate([dR.reshape(-1), dt]), np.concatenate([tdR.reshape(-1), tdt]))
        if "g_cam_unnorm_rots" in v and "sums" in v:
            s32 = v["sums"].astype(F).astype(d)
            g_cq, g_ct = tail64(cq, s32[:9].reshape(3, 3), s32[9:])
            t_cq, _ = tail64(cq, s32[:9].reshape(3, 3), s32[9:], magnitudes=True)
            got = v["g_cam_unnorm_rots"][0, :, time_idx]
            out["tail"] = (got, g_cq, t_cq)
            assert np.array_equal(v["g_cam_trans"][0, :, time_idx], s32[9:])
    if "g_unnorm_rotations" in v:
        g = x["g_rotations"]
        want = (g - rot * (rot * g).sum(1, keepdims=True)) / n
        terms = (np.abs(g) + np.abs(rot) * np.abs(rot * g).sum(1, keepdims=True)) / n
        out["g_unnorm_rotations"] = (v["g_unnorm_rotations"], want, terms)
    if "g_logit_opacities" in v:
        o32 = v["opacities"]
        want = x["g_opacities"] * o32 * (1 - o32)
        out["g_logit_opacities"] = (v["g_logit_opacities"], want, np.abs(want))
    if "g_log_scales" in v:
        prod = x["g_scales"] * v["scales"]
        if x["log_scales"].shape[1] == 1:
            out["g_log_scales"] = (v["g_log_scales"], prod.sum(1, keepdims=True), np.abs(prod).sum(1, keepdims=True))
        else:
            out["g_log_scales"] = (v["g_log_scales"], prod, np.abs(prod))
    return out


def k_need(got, want64, terms):
    """max over the elements of (|got - want64| - 2^-149) / (2^-24 sum|terms|): the K the rule would have to hold"""
    got, want64, terms = (np.asarray(a, np.float64) for a in (got, want64, terms))
    if got.size == 0:
        return 0.0
    if not (np.isfinite(got).all() and np.isfinite(want64).all()):
        return float("inf")
    dev = np.maximum(np.abs(got - want64) - 2.0 ** -149, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        need = np.where(dev == 0, 0.0, dev / (2.0 ** -24 * terms))
    return float(need.max())


def torch32_staged(inp, time_idx):
    """torch's own float32 ops stage by stage on the CPU, every stage fed the float32 result of the one before and differentiated by
    autograd on its own: `vals` for `stages` -- the K that torch's chain needs, stage by stage"""
    t = {k: torch.from_numpy(v) for k, v in inp.items()}
    leaf = lambda a: a.detach().clone().requires_grad_(True)
    cq, ct = leaf(t["cam_unnorm_rots"][..., time_idx]), leaf(t["cam_trans"][..., time_idx])
    rel = t_pose(cq, ct)
    rel_in, means = leaf(rel), leaf(t["means3D"])
    pts = t_points(rel_in, means)
    pts_in = leaf(pts)
    feats = t_feats(t["first_frame_w2c"], pts_in)
    q, lo, ls = leaf(t["unnorm_rotations"]), leaf(t["logit_opacities"]), leaf(t["log_scales"])
    rot, opac, scales = tF.normalize(q), torch.sigmoid(lo), t_scales(ls)
    G = t["g_pts"] + torch.autograd.grad(feats, pts_in, t["g_feats"])[0]
    g_means, g_rel = torch.autograd.grad(pts, [means, rel_in], G)
    g_cq, g_ct = torch.autograd.grad(rel, [cq, ct], g_rel)
    full = lambda g, c: np.stack([g[0].numpy() if k == time_idx else np.zeros(c, F) for k in range(inp["cam_trans"].shape[2])], 1)[None]
    vals = {"rel_w2c": rel, "pts": pts, "feats": feats, "rotations": rot, "opacities": opac, "scales": scales, "G": G, "g_means3D": g_means,
            "sums": torch.cat([g_rel[:3, :3].reshape(-1), g_rel[:3, 3]]),
            "g_unnorm_rotations": torch.autograd.grad(rot, q, t["g_rotations"])[0],
            "g_logit_opacities": torch.autograd.grad(opac, lo, t["g_opacities"])[0],
            "g_log_scales": torch.autograd.grad(scales, ls, t["g_scales"])[0]}
    vals = {k: v.detach().numpy() for k, v in vals.items()}
    vals["g_cam_unnorm_rots"], vals["g_cam_trans"] = full(g_cq, 4), full(g_ct, 3)
    return vals


# ---- the g++ harness over csrc/fr_rendervar_math.h (tests/harness/fr_rendervar_harness.cpp) -----------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_rendervar_harness"))
    vp = ctypes.c_void_p
    h.frv_forward.argtypes = [vp]
    h.frv_forward.restype = None
    h.frv_backward.argtypes = [vp, vp, vp]
    h.frv_backward.restype = None
    h.frv_tail.argtypes = [vp] * 6
    h.frv_tail.restype = None
    h.frv_layout.argtypes = [vp]
    h.frv_layout.restype = None
    return h


def _cfg(arrays, P, scale_cols, time_idx, frames):
    from fisher_rast import _lib
    cfg = _lib.RenderVarCfg(int(P), int(scale_cols), int(time_idx), int(frames))
    for k, a in arrays.items():
        if a is not None:
            assert a.dtype == F and a.flags["C_CONTIGUOUS"], k
            setattr(cfg, k, a.ctypes.data)
    return cfg


def harness_run(h, inp, time_idx, gaussians_grad=True, camera_grad=True, skip=()):
    """forward and backward of the harness on the arrays of `inp`: {name: float32 array} with every output, every gradient the flags
    ask for, 'rel_w2c', 'G' [P,3] and 'sums' [12] (binary64).  Names in `skip` (outputs, upstream gradients or gradients) are null."""
    P, cols, frames = inp["means3D"].shape[0], inp["log_scales"].shape[1], inp["cam_trans"].shape[2]
    ins = {k: inp[k] for k in PARAMS + ("first_frame_w2c",)}
    shapes = {"pts": (P, 3), "feats": (P, 3), "rotations": (P, 4), "opacities": (P, 1), "scales": (P, 3), "rel_w2c": (4, 4)}
    out = {k: np.full(s, 7.0, F) for k, s in shapes.items() if k not in skip}
    h.frv_forward(ctypes.byref(_cfg({**ins, **out}, P, cols, time_idx, frames)))
    gshapes = {"g_means3D": (P, 3) if gaussians_grad else None, "g_unnorm_rotations": (P, 4), "g_logit_opacities": (P, 1), "g_log_scales": (P, cols),
               "g_cam_unnorm_rots": (1, 4, frames) if camera_grad else None, "g_cam_trans": (1, 3, frames) if camera_grad else None}
    grads = {k: np.full(s, 7.0, F) for k, s in gshapes.items() if s is not None and k not in skip}
    G, sums = np.full((P, 3), 7.0, F), np.zeros(12, np.float64)
    ups = {k: inp[k] for k in UPSTREAM if k not in skip}
    h.frv_backward(ctypes.byref(_cfg({**ins, **ups, **grads}, P, cols, time_idx, frames)), G.ctypes.data, sums.ctypes.data)
    return {**out, **grads, "G": G, "sums": sums}


class HarnessBackend:
    """CPU stand-in for fisher_rast.rendervar.HipRenderVarBackend: the same calls, done by the g++ harness on the CPU tensors' memory"""

    def __init__(self, harness):
        self.h = harness
        self.forwards, self.backwards = [], []          # the non-null tensor names of every call

    @staticmethod
    def check(tensors, time_idx):
        from fisher_rast import ops
        return ops.rendervar_check(tensors, time_idx, need_cuda=False)

    def _cfg(self, P, scale_cols, time_idx, n_frames, tensors):
        from fisher_rast import ops
        assert all(t is None or t.device.type == "cpu" for t in tensors.values())
        return ops.rendervar_cfg(P, scale_cols, time_idx, n_frames, tensors)

    def forward(self, P, scale_cols, time_idx, n_frames, tensors):
        self.forwards.append(sorted(k for k, t in tensors.items() if t is not None))
        self.h.frv_forward(ctypes.byref(self._cfg(P, scale_cols, time_idx, n_frames, tensors)))

    def backward(self, P, scale_cols, time_idx, n_frames, tensors):
        self.backwards.append(sorted(k for k, t in tensors.items() if t is not None))
        self.h.frv_backward(ctypes.byref(self._cfg(P, scale_cols, time_idx, n_frames, tensors)), None, None)


# ---- the special rows ---------------------------------------------------------------------------------------------------------------

def special_inputs(scale_cols, seed=5):
    """16 ordinary rows with the special ones written over rows 0 .. 13: a zero Gaussian quaternion, logits +-100, log scales 89 and
    -104, a NaN in each per-Gaussian input and in each upstream gradient"""
    inp = make_inputs(16, scale_cols, seed)
    inp["unnorm_rotations"][0] = 0.0
    inp["logit_opacities"][1], inp["logit_opacities"][2] = 100.0, -100.0
    inp["log_scales"][3, 0], inp["log_scales"][4, -1] = 89.0, -104.0
    inp["means3D"][5, 1] = np.nan
    inp["unnorm_rotations"][6, 2] = np.nan
    inp["logit_opacities"][7, 0] = np.nan
    inp["log_scales"][8, 0] = np.nan
    inp["g_pts"][9, 0] = inp["g_feats"][10, 2] = inp["g_rotations"][11, 1] = inp["g_opacities"][12, 0] = inp["g_scales"][13, 1] = np.nan
    return inp
