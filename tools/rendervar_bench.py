#!/usr/bin/env python3
"""tools/rendervar_bench.py [out.json] [--sizes 20000,2000000] [--no-trace] [--no-iteration] | --kernels-only ROUTE --config mapping|tracking --cols 1|3 --iters K [--size P]

What the stretch between `params` and the rasteriser costs in one tracking / mapping iteration -- transform_to_frame, the (z, 1, z^2)
depth / silhouette features, the normalised rotations, the opacities and the scales, forward and backward with the upstream gradients
given -- on a map of 20k and of 2M Gaussians, isotropic ([P,1]) and anisotropic ([P,3]) scales:
  torch   the chain of torch ops, written out below and in models/SLAM/utils/slam_helpers.py (two normalisations of the camera
          quaternion, nine single-entry fills, eye(4) + two slice assignments, ones / cat / matmul, cat / matmul / square / cat,
          F.normalize / sigmoid / tile + exp), and autograd
  fused   fisher_rast.rendervar.FrameRenderVars (fr_rendervar_forward / fr_rendervar_backward: one launch each way, two backward with
          the camera's gradient)
mapping: the Gaussians take the gradient; tracking: the camera pose does (and the three activations' parameters, as in the
reference).  Per route: ITERS forward + backward between two device events (event ms) and inside a host clock that ends in a device
synchronise (wall ms); REPS alternating repeats after a warm-up; median [min .. max].  Host synchronisations are what torch's sync debug
mode reports during one forward + backward.

One mapping iteration at the shape of tools/config4_train_step.py (2M Gaussians, 512x512) through make_get_loss with
fused_rendervar on and off (--no-iteration leaves it out).

Launch counts come from kernel traces in child processes of their own, after the timing: per route the tool runs
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/rendervar_bench.py --kernels-only <route> --config <c> --cols <n> --iters 10
and the same with --iters 20; (kernels in the second trace - kernels in the first) / 10 = launches per forward + backward.  --no-trace
leaves that out."""
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
from fisher_rast.rendervar import FrameRenderVars    # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS = 7
FRAMES = 100
TIME_IDX = 37
PARAMS = ("means3D", "unnorm_rotations", "logit_opacities", "log_scales", "cam_unnorm_rots", "cam_trans")


# ---- the torch chain, op for op ------------------------------------------------------------------------------------------------------

def rotation_of(quat):
    """[N,3,3] rotation matrices of the quaternions [N,4] (w first).  The op structure is the one being priced: the argument is
    normalised here once more, by the root of its four squared components, and the nine entries are written one at a time into a
    zero matrix -- each entry a handful of launches."""
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


def torch_transform_to_frame(params, time_idx, gaussians_grad, camera_grad):
    """the means in the frame of camera `time_idx` by torch ops: F.normalize of the frame's quaternion, `rotation_of`, an identity
    4 x 4 with the rotation and the translation assigned into it, a column of ones appended to the means, one matmul"""
    quat, shift = params['cam_unnorm_rots'][..., time_idx], params['cam_trans'][..., time_idx]
    if not camera_grad:
        quat, shift = quat.detach(), shift.detach()
    pose = torch.eye(4, device=dev)
    pose[:3, :3] = rotation_of(F.normalize(quat))
    pose[:3, 3] = shift
    means = params['means3D'] if gaussians_grad else params['means3D'].detach()
    homogeneous = torch.cat((means, torch.ones((means.shape[0], 1), device=dev)), dim=1)
    return (pose @ homogeneous.T).T[:, :3]


def torch_chain(params, w2c, gaussians_grad, camera_grad):
    from models.SLAM.utils.slam_helpers import get_depth_and_silhouette
    pts = torch_transform_to_frame(params, TIME_IDX, gaussians_grad, camera_grad)
    log_scales = params['log_scales']
    return (pts, get_depth_and_silhouette(pts, w2c), F.normalize(params['unnorm_rotations']), torch.sigmoid(params['logit_opacities']),
            torch.exp(log_scales if log_scales.shape[-1] == 3 else torch.tile(log_scales, (1, 3))))


def fused_chain(params, w2c, gaussians_grad, camera_grad):
    return FrameRenderVars.apply(params['means3D'], params['unnorm_rotations'], params['logit_opacities'], params['log_scales'],
                                 params['cam_unnorm_rots'], params['cam_trans'], TIME_IDX, w2c, gaussians_grad, camera_grad)


CHAINS = dict(torch=torch_chain, fused=fused_chain)


def make(P, cols, config, route, seed=7):
    """a forward + backward of `route` on its own parameters, the upstream gradients given"""
    g = torch.Generator().manual_seed(seed)
    shapes = dict(means3D=(P, 3), unnorm_rotations=(P, 4), logit_opacities=(P, 1), log_scales=(P, cols), cam_unnorm_rots=(1, 4, FRAMES),
                  cam_trans=(1, 3, FRAMES))
    params = {k: torch.randn(s, generator=g).to(dev).requires_grad_(True) for k, s in shapes.items()}
    w2c = torch.eye(4, device=dev)
    up = [torch.randn(s, generator=g).to(dev) for s in ((P, 3), (P, 3), (P, 4), (P, 1), (P, 3))]
    gg, cg = config == "mapping", config == "tracking"
    chain = CHAINS[route]

    def step():
        torch.autograd.backward(chain(params, w2c, gg, cg), up)
        for v in params.values():
            v.grad = None

    return step


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
        for _ in range(3):
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


def traced_kernels(route, config, cols, iters, P):
    """(kernels, kernels named k_rendervar_*) in a kernel trace of a child process that makes `iters` forward + backward"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--kernels-only", route, "--config", config, "--cols", str(cols), "--iters", str(iters), "--size", str(P)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        with open(files[0]) as f:
            names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return len(names), sum("k_rendervar" in n for n in names)


def mapping_iteration(P, W, H, lines):
    """ms per mapping iteration of make_get_loss (fused render pair, fused loss) -> backward, with fused_rendervar off and on"""
    from fisher_rast import synthetic
    from models.SLAM.gaussian import make_get_loss
    from models.SLAM.utils import slam_helpers as sh
    from models.SLAM.utils.recon_helpers import setup_camera
    init = {k: v.contiguous() for k, v in synthetic.room_shell(P, 4).items()}
    init["cam_unnorm_rots"] = torch.tensor([[[1.0], [0.0], [0.0], [0.0]]])
    init["cam_trans"] = torch.zeros((1, 3, 1))
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=dev)
    gen = torch.Generator().manual_seed(44)
    curr = dict(cam=cam, w2c=torch.eye(4, device=dev), im=torch.rand((3, H, W), generator=gen).to(dev),
                depth=(1.0 + 3.0 * torch.rand((1, H, W), generator=gen)).to(dev))
    weights = dict(im=0.5, depth=1.0)
    routes = {}
    for route in ("torch", "fused"):
        params = {k: v.to(dev).requires_grad_(True) for k, v in init.items()}
        variables = dict(max_2D_radius=torch.zeros(P, device=dev), means2D_gradient_accum=torch.zeros(P, device=dev), denom=torch.zeros(P, device=dev))
        get_loss = make_get_loss(torch_transform_to_frame, sh.calc_loss, fused_rendervar=(route == "fused"))

        def step(params=params, variables=variables, get_loss=get_loss):
            loss, _, _ = get_loss(params, curr, variables, 0, weights, True, 0.5, True, False, mapping=True)
            loss.backward()
            for v in params.values():
                v.grad = None

        routes[route] = step
    res = compare(routes, 10)
    for k in ("torch", "fused"):
        e, w = res[k]["event_ms"], res[k]["wall_ms"]
        lines.append(f"mapping iteration P={P} {W}x{H}  render variables {k:5s}  event {e['median']:.3f} ms [{e['min']:.3f} .. {e['max']:.3f}]   "
                     f"wall {w['median']:.3f} ms [{w['min']:.3f} .. {w['max']:.3f}]")
    res["saved_event_ms"] = res["torch"]["event_ms"]["median"] - res["fused"]["event_ms"]["median"]
    res["fused_range_below_torch_range_event_ms"] = res["fused"]["event_ms"]["max"] < res["torch"]["event_ms"]["min"]
    lines.append(f"mapping iteration P={P} {W}x{H}  torch - fused = {res['saved_event_ms']:.3f} ms per iteration (event); "
                 f"whole range below torch's: {res['fused_range_below_torch_range_event_ms']}")
    return res


if "--kernels-only" in sys.argv:
    route, config, cols = _opt("--kernels-only"), _opt("--config", "mapping"), int(_opt("--cols", "3"))
    iters, P = int(_opt("--iters", "10")), int(_opt("--size", "20000"))
    step = make(P, cols, config, route)
    for _ in range(iters):
        step()
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, config=config, cols=cols, iters=iters, size=P)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]


def save():
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


sizes = [int(s) for s in _opt("--sizes", "20000,2000000").split(",")]
out = dict(what="forward + backward of the render-variable build (upstream gradients given): the torch chain against FrameRenderVars; "
                "ms per forward + backward, median [min .. max] of 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, cases={})
lines = []
for P in sizes:
    iters = 100 if P <= 100000 else 10
    for config in ("mapping", "tracking"):
        for cols in (1, 3):
            made = {r: make(P, cols, config, r) for r in ("torch", "fused")}
            res = compare(made, iters)
            res["iters"] = iters
            res["host_syncs"] = {r: host_syncs(made[r]) for r in made}
            for r in made:
                e, w = res[r]["event_ms"], res[r]["wall_ms"]
                lines.append(f"{config:8s} P={P} scale columns {cols}  {r:5s}  event {e['median']:.4f} ms [{e['min']:.4f} .. {e['max']:.4f}]   "
                             f"wall {w['median']:.4f} ms [{w['min']:.4f} .. {w['max']:.4f}]   host syncs {res['host_syncs'][r]}")
            for what in ("event_ms", "wall_ms"):
                res[f"torch_over_fused_{what}"] = res["torch"][what]["median"] / res["fused"][what]["median"]
                res[f"fused_range_below_torch_range_{what}"] = res["fused"][what]["max"] < res["torch"][what]["min"]
            lines.append(f"{config:8s} P={P} scale columns {cols}  torch / fused = {res['torch_over_fused_event_ms']:.2f}x (event), "
                         f"{res['torch_over_fused_wall_ms']:.2f}x (wall); whole range below torch's: {res['fused_range_below_torch_range_event_ms']}")
            out["cases"][f"{config}/{P}/{cols}"] = res
            del made
            torch.cuda.empty_cache()
if "--no-iteration" not in sys.argv:
    out["mapping_iteration"] = mapping_iteration(2_000_000, 512, 512, lines)
    torch.cuda.empty_cache()
save()                                   # the timings are on file before the traces start
if "--no-trace" not in sys.argv:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on the PATH: the launch counts cannot be traced (--no-trace leaves them out)")
    for config in ("mapping", "tracking"):
        for cols in (1, 3):
            n = out["cases"][f"{config}/{sizes[0]}/{cols}"]["launches_per_call"] = {}
            for r in ("torch", "fused"):
                a, b = traced_kernels(r, config, cols, 10, sizes[0]), traced_kernels(r, config, cols, 20, sizes[0])
                n[r] = dict(all=(b[0] - a[0]) / 10.0, rendervar_kernels=(b[1] - a[1]) / 10.0)
            lines.append(f"launches per forward + backward, {config} P={sizes[0]} scale columns {cols} (kernel trace, runs of 10 and 20, difference / 10): "
                         f"torch {n['torch']['all']:.0f}, fused {n['fused']['all']:.0f} ({n['fused']['rendervar_kernels']:.0f} k_rendervar_*)")
    save()
print("\n".join(lines))
print(json.dumps(out))
