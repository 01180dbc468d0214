#!/usr/bin/env python3
"""tools/frame_ingest_bench.py [out.json] | --kernels-only fused|torch --iters K [--size S] [--downsample D]

What the frame ingest (fr_frame_ingest_select / fr_frame_ingest_emit) costs against the torch chain it replaces: one
`add_new_gaussians` of the mapping loop on a 20k-Gaussian map that covers the left half of an S x S frame (so about half the
frame is non-present), S = 256 and 512, downsample 1 and 4, isotropic off, add_rand_gaussians off (as in every shipped config).
  fused   models/SLAM/gaussian.add_new_gaussians of this package (depth / silhouette render, select, one host read, emit)
  torch   the chain the reference runs (models/SLAM/gaussian.py:320-414 over 75-143 and 299-318), written out below in this
          tool's own form: the same render, then abs / median / compare, `sum() > 0`, meshgrid, torch.inverse, matmul, max_pool2d,
          `sum() > 0`, two boolean indexings, log / sqrt / tile, a cat per parameter.  The reference's print of the scale range (two
          more host reads) is left out of both.
Both routes render with the same rasteriser and start every iteration from the same map.  Per route: ITERS iterations between two
device events (event ms / iteration) and inside a host clock that ends in a device synchronise (wall ms / iteration); REPS
alternating repeats after a warm-up; median [min .. max].  Host synchronisations per call are what torch's sync debug mode reports
during one call.

Launch counts come from kernel traces in child processes of their own, after the timing (tracing slows the host): per route the
tool runs
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/frame_ingest_bench.py --kernels-only <route> --iters 10
and the same with --iters 20; (kernels in the second trace - kernels in the first) / 10 = launches per call, the render, the
transform to the frame and the copies of the old rows included.  The kernels of this library among them are counted by name.
--no-trace leaves that part out."""
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
from diff_gaussian_rasterization import GaussianRasterizer as Renderer               # noqa: E402
from models.SLAM import gaussian as G                                                # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera                             # noqa: E402
from models.SLAM.utils.slam_helpers import transformed_params2depthplussilhouette    # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, ITERS, P = 7, 100, 20000
SIL_THRES, RATIO, TIME_IDX = 0.5, 50.0, 1


def make_frame(S, seed=7):
    """(params, variables, curr_data): Gaussians over the left half of the view of frame 1, a full RGB-D frame"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(1.0, 4.0, P)
    means = np.stack([rng.uniform(-1.0, 0.0, P) * z, rng.uniform(-1.0, 1.0, P) * z, z], 1)
    rot = rng.normal(size=(P, 4))
    params = dict(means3D=means, rgb_colors=rng.uniform(0, 1, (P, 3)), unnorm_rotations=rot / np.linalg.norm(rot, axis=1, keepdims=True),
                  logit_opacities=rng.normal(2.0, 1.0, (P, 1)), log_scales=np.log(0.04 * z)[:, None].repeat(3, 1) + rng.normal(0, 0.2, (P, 3)),
                  cam_unnorm_rots=np.stack([[1.0, 0, 0, 0], [1.0, 0.004, -0.006, 0.003]], -1)[None],
                  cam_trans=np.stack([[0.0, 0, 0], [0.01, -0.005, 0.008]], -1)[None])
    params = {k: torch.nn.Parameter(torch.tensor(v, dtype=torch.float32, device=dev).contiguous().requires_grad_(True)) for k, v in params.items()}
    variables = {k: torch.zeros(P, device=dev) for k in ("max_2D_radius", "means2D_gradient_accum", "denom", "timestep")}
    K = np.array([[S / 2.0, 0, S / 2.0], [0, S / 2.0, S / 2.0], [0, 0, 1]], np.float32)
    curr = dict(cam=setup_camera(S, S, K, np.eye(4), device=dev), w2c=torch.eye(4, device=dev), intrinsics=torch.from_numpy(K).to(dev),
                im=torch.from_numpy(rng.uniform(0, 1, (3, S, S)).astype(np.float32)).to(dev),
                depth=torch.from_numpy(rng.uniform(1.0, 4.0, (1, S, S)).astype(np.float32)).to(dev))
    return params, variables, curr


def torch_get_pointcloud(color, depth, intrinsics, w2c, downsample, mask):
    H, W = color.shape[1], color.shape[2]
    cx, cy, fx, fy = intrinsics[0][2], intrinsics[1][2], intrinsics[0][0], intrinsics[1][1]
    xg, yg = torch.meshgrid(torch.arange(0, W, step=downsample, device=dev).float(), torch.arange(0, H, step=downsample, device=dev).float(), indexing="xy")
    xx, yy = ((xg - cx) / fx).reshape(-1), ((yg - cy) / fy).reshape(-1)
    z = depth[0, ::downsample, ::downsample].reshape(-1)
    cam = torch.stack((xx * z, yy * z, z), dim=-1)
    pts4 = torch.cat((cam, torch.ones(cam.shape[0], 1, device=dev)), dim=1)
    pts = (torch.inverse(w2c) @ pts4.T).T[:, :3]
    msd = (downsample * z / ((fx + fy) / 2)) ** 2
    cols = color[:, ::downsample, ::downsample].permute(1, 2, 0).reshape(-1, 3)
    cld = torch.cat((pts, cols), -1)
    keep = F.max_pool2d(mask.reshape(1, H, W).float(), downsample).bool().reshape(-1)
    if keep.sum() > 0:
        cld, msd = cld[keep], msd[keep]
    return cld, msd


def torch_add_new_gaussians(config, params, variables, curr_data, sil_thres, time_idx, mean_sq_dist_method, densify_dict,
                            add_rand_gaussians=True, downsample_pcd=1):
    """the chain this package's add_new_gaussians replaces (add_rand_gaussians off)"""
    pts = G._transform_to_frame(params, time_idx, gaussians_grad=False, camera_grad=False)
    depth_sil, _, _ = Renderer(raster_settings=curr_data['cam'])(**transformed_params2depthplussilhouette(params, curr_data['w2c'], pts))
    sil, render, gt = depth_sil[1], depth_sil[0], curr_data['depth'][0]
    err = torch.abs(gt - render) * (gt > 0)
    mask = (sil < sil_thres) | ((render > gt) * (err > densify_dict["depth_error_ratio"] * err.median()))
    mask = mask.reshape(-1) & (gt > 0.01).reshape(-1)
    if torch.sum(mask) > 0:
        cld, msd = torch_get_pointcloud(curr_data['im'], curr_data['depth'], curr_data['intrinsics'], G.frame_w2c(params, time_idx), downsample_pcd, mask)
        n = cld.shape[0]
        rots = torch.zeros((n, 4), device=dev)
        rots[:, 0] = 1
        new = dict(means3D=cld[:, :3], rgb_colors=cld[:, 3:6], unnorm_rotations=rots, logit_opacities=torch.zeros((n, 1), device=dev),
                   log_scales=torch.tile(torch.log(torch.sqrt(msd))[..., None], (1, 1 if config["isotropic"] else 3)))
        for k, v in new.items():
            v = torch.nn.Parameter(v.float().contiguous().requires_grad_(True))
            params[k] = torch.nn.Parameter(torch.cat((params[k], v), dim=0).requires_grad_(True))
        total = params['means3D'].shape[0]
        for k in ('means2D_gradient_accum', 'denom', 'max_2D_radius'):
            variables[k] = torch.zeros(total, device=dev)
        variables['timestep'] = torch.cat((variables['timestep'], time_idx * torch.ones(n, device=dev)), dim=0)
    return params, variables


ROUTES = dict(fused=G.add_new_gaussians, torch=torch_add_new_gaussians)


def call(fn, frame, d):
    params, variables, curr = frame
    return fn(dict(isotropic=False), dict(params), dict(variables), curr, SIL_THRES, TIME_IDX, "projective", dict(depth_error_ratio=RATIO),
              add_rand_gaussians=False, downsample_pcd=d)


def timed(step, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, 1e3 * (time.perf_counter() - t0) / iters


def compare(routes, iters):
    for step in routes.values():
        for _ in range(5):
            step()
    torch.cuda.synchronize()
    raw = {k: [] for k in routes}
    for _ in range(REPS):
        for k, step in routes.items():
            raw[k].append(timed(step, iters))
    out = {}
    for k, v in raw.items():
        out[k] = {}
        for j, what in enumerate(("event_ms", "wall_ms")):
            s = sorted(t[j] for t in v)
            out[k][what] = dict(median=s[len(s) // 2], min=s[0], max=s[-1])
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


def traced_kernels(route, iters, S, d):
    """(kernels, kernels named k_ingest_*) in a kernel trace of a child process that makes `iters` calls"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--kernels-only", route, "--iters", str(iters), "--size", str(S), "--downsample", str(d)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        with open(files[0]) as f:
            names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return len(names), sum("k_ingest_" in n for n in names)


def launches_per_call(S, d):
    out = {}
    for route in ROUTES:
        (a, ai), (b, bi) = traced_kernels(route, 10, S, d), traced_kernels(route, 20, S, d)
        out[route] = dict(all=(b - a) / 10.0, ingest_kernels=(bi - ai) / 10.0)
    return out


if "--kernels-only" in sys.argv:
    route, iters = _opt("--kernels-only"), int(_opt("--iters", "10"))
    S, d = int(_opt("--size", "256")), int(_opt("--downsample", "1"))
    frame = make_frame(S)
    for _ in range(iters):
        call(ROUTES[route], frame, d)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, iters=iters, size=S, downsample=d)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]
out = dict(what="one add_new_gaussians (depth / silhouette render of a 20k-Gaussian map over half the frame, selection, new parameter rows), "
                "fused frame ingest against the torch chain; ms per call, median [min .. max] of 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, iters=ITERS, P=P, cases={})
lines = []
for S in (256, 512):
    frame = make_frame(S)
    for d in (1, 4):
        res = compare({k: (lambda fn=fn: call(fn, frame, d)) for k, fn in ROUTES.items()}, ITERS)
        (pa, va), (pb, vb) = call(ROUTES["fused"], frame, d), call(ROUTES["torch"], frame, d)
        n_new = int(pa["means3D"].shape[0]) - P
        res["new_gaussians"] = dict(fused=n_new, torch=int(pb["means3D"].shape[0]) - P, grid=(S // d) ** 2)
        res["rows_agree"] = bool(pa["means3D"].shape == pb["means3D"].shape and torch.equal(pa["rgb_colors"], pb["rgb_colors"])
                                 and torch.allclose(pa["means3D"], pb["means3D"], rtol=1e-5, atol=1e-5)
                                 and torch.allclose(pa["log_scales"], pb["log_scales"], rtol=1e-6, atol=1e-6) and torch.equal(va["timestep"], vb["timestep"]))
        res["host_syncs"] = {k: host_syncs(lambda fn=fn: call(fn, frame, d)) for k, fn in ROUTES.items()}
        for what in ("event_ms", "wall_ms"):
            res[f"torch_over_fused_{what}"] = res["torch"][what]["median"] / res["fused"][what]["median"]
            res[f"fused_range_below_torch_range_{what}"] = res["fused"][what]["max"] < res["torch"][what]["min"]
        out["cases"][f"{S}/d{d}"] = res
        tag = f"add_new_gaussians {S}x{S} d={d} ({n_new} of {(S // d) ** 2} cells)"
        for k in ("fused", "torch"):
            e, w = res[k]["event_ms"], res[k]["wall_ms"]
            lines.append(f"{tag}  {k:5s}  event {e['median']:.4f} ms [{e['min']:.4f} .. {e['max']:.4f}]   "
                         f"wall {w['median']:.4f} ms [{w['min']:.4f} .. {w['max']:.4f}]   host syncs {res['host_syncs'][k]}")
        lines.append(f"{tag}  torch / fused = {res['torch_over_fused_event_ms']:.2f}x (event), {res['torch_over_fused_wall_ms']:.2f}x (wall); "
                     f"rows agree: {res['rows_agree']}")
if "--no-trace" not in sys.argv:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on the PATH: the launch counts cannot be traced (--no-trace leaves them out)")
    for S, d in ((256, 1), (512, 4)):
        n = out["cases"][f"{S}/d{d}"]["launches_per_call"] = launches_per_call(S, d)
        lines.append(f"launches per add_new_gaussians {S}x{S} d={d} (kernel trace, runs of 10 and 20 calls, difference / 10): "
                     f"fused {n['fused']['all']:.0f} ({n['fused']['ingest_kernels']:.0f} of them the ingest kernels; the rest the render, the transform to "
                     f"the frame, the pose and the copies of the old rows), torch {n['torch']['all']:.0f}")
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
