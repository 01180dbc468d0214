#!/usr/bin/env python3
"""tools/keyframe_select_bench.py [out.json] | --kernels-only fused|torch --iters N [--size S] [--keyframes K] [--masks 0|1]

What the keyframe selection (fr_keyframe_valid_pixels / fr_keyframe_overlap under models/SLAM/utils/keyframe_selection.py) costs
against the torch chain it replaces: one `keyframe_selection_overlap` of the mapping loop on an S x S depth frame with 5 % of the
pixels unmeasured, S = 256 and 512, K = 8, 64 and 256 keyframes around the current pose, pixels = 1600, k = 10, with and without a
keyframe object mask on every keyframe.
  fused   this package's drop-in: two library calls, two host reads
  torch   the chain the reference runs (models/SLAM/utils/keyframe_selection.py:10-37, 40-134), written out below in this tool's own
          form: torch.where, unique / isin, torch.inverse, about fifteen small launches per keyframe in a Python loop, a Python sort
          of 0-dim device tensors
Both routes run in this process under the same seeds.  Per route: ITERS calls inside a host clock that ends in a device synchronise
(wall ms / call); REPS alternating repeats after a warm-up; median [min .. max].  Host synchronisations per call are what torch's
sync debug mode reports during one call.

Launch counts come from kernel traces in child processes of their own, after the timing (tracing slows the host): per route the
tool runs
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/keyframe_select_bench.py --kernels-only <route> --iters 5
and the same with --iters 10; (kernels in the second trace - kernels in the first) / 5 = launches per call.  The kernels of this
library among them are counted by name.  --no-trace leaves that part out."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import torch.nn.functional as F   # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from models.SLAM.utils import keyframe_selection as ks                               # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, ITERS, PIXELS, K_ASKED = 5, 20, 1600, 10


def _rigid(yaw, pitch, t):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    m = np.eye(4)
    m[:3, :3] = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    m[:3, 3] = t
    return m


def make_scene(S, K, masks, seed=7):
    """(gt_depth [1,S,S], w2c, intrinsics, keyframe_list) on the device"""
    rng = np.random.default_rng([S, K, int(masks), seed])
    depth = rng.uniform(1.0, 4.0, (1, S, S)).astype(np.float32)
    depth[rng.uniform(size=depth.shape) < 0.05] = 0.0
    intr = np.array([[0.6 * S, 0, 0.5 * S], [0, 0.6 * S, 0.5 * S], [0, 0, 1]], np.float32)
    w2c = _rigid(0.3, 0.0, (0.2, -0.1, 0.3))
    kfs = []
    for _ in range(K):
        pose = _rigid(rng.uniform(-0.6, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(-0.5, 0.5, 3)) @ w2c
        kf = dict(est_w2c=torch.from_numpy(pose.astype(np.float32)).to(dev))
        if masks:
            coarse = rng.uniform(size=(S // 16, S // 16)) < 0.6
            kf["obj_mask_2d"] = torch.from_numpy(np.repeat(np.repeat(coarse, 16, 0), 16, 1)).to(dev)
        kfs.append(kf)
    return torch.from_numpy(depth).to(dev), torch.from_numpy(w2c.astype(np.float32)).to(dev), torch.from_numpy(intr).to(dev), kfs


def torch_get_pointcloud(depth, intrinsics, w2c, rowcol):
    fx, fy, cx, cy = intrinsics[0][0], intrinsics[1][1], intrinsics[0][2], intrinsics[1][2]
    z = depth[0, rowcol[:, 0], rowcol[:, 1]]
    cam = torch.stack(((rowcol[:, 1] - cx) / fx * z, (rowcol[:, 0] - cy) / fy * z, z), dim=-1)
    cam4 = torch.cat([cam, torch.ones_like(cam[:, :1])], dim=1).float()
    pts = (torch.inverse(w2c) @ cam4.T).T[:, :3]
    keys = torch.abs(torch.round(pts, decimals=4))
    zero = torch.zeros((1, 3), device=pts.device)
    _, inverse, counts = torch.cat([keys, zero], dim=0).unique(dim=0, return_inverse=True, return_counts=True)
    repeated = torch.isin(inverse, torch.where(counts.gt(1))[0])[:len(keys)]
    return pts[~repeated]


def torch_keyframe_selection_overlap(gt_depth, w2c, intrinsics, keyframe_list, k, curr_mask=None, pixels=1600):
    """the chain this package's keyframe_selection_overlap replaces"""
    H, W, edge = gt_depth.shape[1], gt_depth.shape[2], 20
    ok = gt_depth[0] > 0
    if curr_mask is not None:
        ok = ok & curr_mask.bool()
    rowcol = torch.stack(torch.where(ok), dim=1)
    if rowcol.shape[0] == 0:
        return []
    draws = torch.randint(rowcol.shape[0], (min(pixels, rowcol.shape[0]),))
    pts = torch_get_pointcloud(gt_depth, intrinsics, w2c, rowcol[draws])
    entries = []
    for i, kf in enumerate(keyframe_list):
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
                m = F.interpolate(m[None, None].float(), size=(H, W), mode="nearest")[0, 0].bool()
            ins = ins & m[uv[:, 1].round().long().clamp(0, H - 1), uv[:, 0].round().long().clamp(0, W - 1)]
        entries.append((i, ins.sum() / uv.shape[0]))
    entries = sorted(entries, key=lambda e: e[1], reverse=True)
    chosen = [i for i, p in entries if p > 0.0]
    return list(np.random.permutation(np.array(chosen))[:k])


ROUTES = dict(fused=ks.keyframe_selection_overlap, torch=torch_keyframe_selection_overlap)


def call(fn, scene, seed=3):
    depth, w2c, intr, kfs = scene
    torch.manual_seed(seed)
    np.random.seed(seed)
    return fn(depth, w2c, intr, kfs, K_ASKED, pixels=PIXELS)


def timed(step, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters


def compare(routes, iters):
    for step in routes.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    raw = {k: [] for k in routes}
    for _ in range(REPS):
        for k, step in routes.items():
            raw[k].append(timed(step, iters))
    out = {}
    for k, v in raw.items():
        s = sorted(v)
        out[k] = dict(wall_ms=dict(median=s[len(s) // 2], min=s[0], max=s[-1]))
    return out


def host_syncs(step):
    """synchronisations torch's sync debug mode reports during one call"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


def traced_kernels(route, iters, S, K, masks):
    """(kernels, kernels named k_kf_*) in a kernel trace of a child process that makes `iters` calls"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--kernels-only", route, "--iters", str(iters), "--size", str(S), "--keyframes", str(K), "--masks", str(int(masks))],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        with open(files[0]) as f:
            names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return len(names), sum("k_kf_" in n for n in names)


def launches_per_call(S, K, masks):
    out = {}
    for route in ROUTES:
        (a, ai), (b, bi) = traced_kernels(route, 5, S, K, masks), traced_kernels(route, 10, S, K, masks)
        out[route] = dict(all=(b - a) / 5.0, keyframe_kernels=(bi - ai) / 5.0)
    return out


if "--kernels-only" in sys.argv:
    route, iters = _opt("--kernels-only"), int(_opt("--iters", "5"))
    S, K, masks = int(_opt("--size", "256")), int(_opt("--keyframes", "8")), bool(int(_opt("--masks", "0")))
    scene = make_scene(S, K, masks)
    for _ in range(iters):
        call(ROUTES[route], scene)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, iters=iters, size=S, keyframes=K, masks=masks)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]
out = dict(what="one keyframe_selection_overlap (pixels = 1600, k = 10) on an S x S depth frame against K keyframes, the HIP drop-in against "
                "the torch chain; wall ms per call (host clock around synchronised calls), median [min .. max] of 5 alternating repeats "
                "of 20 calls after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, iters=ITERS, pixels=PIXELS, cases={})
lines = []
for S in (256, 512):
    for K in (8, 64, 256):
        for masks in (False, True):
            scene = make_scene(S, K, masks)
            res = compare({k: (lambda fn=fn: call(fn, scene)) for k, fn in ROUTES.items()}, ITERS)
            a, b = call(ROUTES["fused"], scene), call(ROUTES["torch"], scene)
            res["selected"] = dict(fused=[int(i) for i in a], torch=[int(i) for i in b])
            res["lists_agree"] = res["selected"]["fused"] == res["selected"]["torch"]
            res["overlapping_keyframes"] = int((ks._hip.last["counts"] > 0).sum())
            res["kept_points"] = ks._hip.last["n_valid"]
            res["host_syncs"] = {k: host_syncs(lambda fn=fn: call(fn, scene)) for k, fn in ROUTES.items()}
            res["torch_over_fused_wall_ms"] = res["torch"]["wall_ms"]["median"] / res["fused"]["wall_ms"]["median"]
            res["fused_range_below_torch_range"] = res["fused"]["wall_ms"]["max"] < res["torch"]["wall_ms"]["min"]
            out["cases"][f"{S}/K{K}/{'masks' if masks else 'nomasks'}"] = res
            tag = f"keyframe_selection_overlap {S}x{S} K={K} {'masks   ' if masks else 'no masks'}"
            for k in ("fused", "torch"):
                w = res[k]["wall_ms"]
                lines.append(f"{tag}  {k:5s}  wall {w['median']:.4f} ms [{w['min']:.4f} .. {w['max']:.4f}]   host syncs {res['host_syncs'][k]}")
            lines.append(f"{tag}  torch / fused = {res['torch_over_fused_wall_ms']:.2f}x (wall); lists agree: {res['lists_agree']} "
                         f"({res['overlapping_keyframes']} of {K} keyframes overlap, {res['kept_points']} of {PIXELS} points kept)")
if "--no-trace" not in sys.argv:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on the PATH: the launch counts cannot be traced (--no-trace leaves them out)")
    for S, K, masks in ((256, 8, False), (256, 256, True)):
        n = out["cases"][f"{S}/K{K}/{'masks' if masks else 'nomasks'}"]["launches_per_call"] = launches_per_call(S, K, masks)
        lines.append(f"launches per keyframe_selection_overlap {S}x{S} K={K} {'masks' if masks else 'no masks'} (kernel trace, runs of 5 and 10 calls, "
                     f"difference / 5): fused {n['fused']['all']:.0f} ({n['fused']['keyframe_kernels']:.0f} of them this library's k_kf_* kernels; the "
                     f"rest the stack of the poses, the concatenation of the two results and copies), torch {n['torch']['all']:.0f}")
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
