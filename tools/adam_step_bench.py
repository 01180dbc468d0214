#!/usr/bin/env python3
"""tools/adam_step_bench.py [out.json] [--sizes 20000,2000000] [--no-trace] [--no-iteration] | --kernels-only ROUTE --config mapping|tracking --iters K [--size P]

What optimizer.step() costs in the reference's two optimizer configurations (get_optimizer, models/SLAM/gaussian.py:1458-1469:
seven groups of one tensor, default learning rates of configs/base_config.py), on a map of 20k and of 2M Gaussians:
  torch       torch.optim.Adam as the reference builds it
  fused       fisher_rast.optim.FusedAdam (fr_adam_step: one launch over the table of every parameter with a gradient)
  fused_skip  FusedAdam(skip_frozen=True), tracking only: the lr == 0 groups -- the whole map -- are left out of the step
mapping: the five map arrays have gradients (14 elements per Gaussian: means 3, colours 3, rotations 4, opacity 1, scales 3), the
camera arrays none.  tracking: all seven arrays have gradients, the five map arrays are frozen (lr == 0).  Per route: ITERS steps
between two device events (event ms / step) and inside a host clock that ends in a device synchronise (wall ms / step); REPS
alternating repeats after a warm-up; median [min .. max].  Achieved bytes/s: 28 B (read p, g, m, v; write p, m, v) per element
the route steps, over the event time -- a whole-step rate, beside the 6.29 TB/s copy rate of the MI355X.  Host synchronisations per
step are what torch's sync debug mode reports during one step.

One mapping iteration at the shape of tools/config4_train_step.py (2M Gaussians, 512x512): render pair -> L1 losses -> backward ->
optimizer.step() -> zero_grad, with the torch optimizer and with the fused one (--no-iteration leaves it out).

Launch counts come from kernel traces in child processes of their own, after the timing (tracing slows the host): per route the tool runs
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/adam_step_bench.py --kernels-only <route> --config <c> --iters 10
and the same with --iters 20; (kernels in the second trace - kernels in the first) / 10 = launches per step.  --no-trace leaves that out."""
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
import __graft_entry__ as entry   # noqa: E402

entry.build()
from fisher_rast.optim import FusedAdam    # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS = 7
COPY_RATE = 6.29e12
MAP_SHAPES = dict(means3D=3, rgb_colors=3, unnorm_rotations=4, logit_opacities=1, log_scales=3)
FRAMES = 100
LRS = {
    "mapping": dict(cam_trans=0.0, cam_unnorm_rots=0.0, log_scales=0.01, logit_opacities=0.05, means3D=0.001, rgb_colors=0.0025, unnorm_rotations=0.001),
    "tracking": dict(cam_trans=0.002, cam_unnorm_rots=0.0004, log_scales=0.0, logit_opacities=0.0, means3D=0.0, rgb_colors=0.0, unnorm_rotations=0.0),
}
ROUTES = {"mapping": ("torch", "fused"), "tracking": ("torch", "fused", "fused_skip")}


def make(P, config, route, seed=7):
    """(optimizer, elements it steps): parameters with the gradients of the configuration in place"""
    g = torch.Generator().manual_seed(seed)
    shapes = {k: (P, c) for k, c in MAP_SHAPES.items()}
    shapes.update(cam_unnorm_rots=(1, 4, FRAMES), cam_trans=(1, 3, FRAMES))
    params = {k: torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for k, s in shapes.items()}
    groups = [{"params": [v], "name": k, "lr": LRS[config][k]} for k, v in params.items()]
    kw = {} if config == "tracking" else dict(lr=0.0, eps=1e-15)
    opt = torch.optim.Adam(groups, **kw) if route == "torch" else FusedAdam(groups, skip_frozen=(route == "fused_skip"), **kw)
    elements = 0
    for k, v in params.items():
        if config == "tracking" or k in MAP_SHAPES:
            v.grad = (torch.randn(shapes[k], generator=g) * 1e-3).to(dev)
            if not (route == "fused_skip" and LRS[config][k] == 0):
                elements += v.numel()
    return opt, elements


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


def traced_kernels(route, config, iters, P):
    """(kernels, kernels named k_adam_step) in a kernel trace of a child process that makes `iters` steps"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--kernels-only", route, "--config", config, "--iters", str(iters), "--size", str(P)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        with open(files[0]) as f:
            names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return len(names), sum("k_adam_step" in n for n in names)


def mapping_iteration(P, W, H, lines):
    """ms per iteration of render pair -> L1 losses -> backward -> optimizer.step() -> zero_grad, torch optimizer against the fused one"""
    from fisher_rast import synthetic
    from models.SLAM.utils.recon_helpers import setup_camera
    from models.SLAM.utils.slam_helpers import render_rgb_depth_sil
    init = {k: v.contiguous() for k, v in synthetic.room_shell(P, 4).items()}
    init["cam_unnorm_rots"] = torch.tensor([[[1.0], [0.0], [0.0], [0.0]]])
    init["cam_trans"] = torch.zeros((1, 3, 1))
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=dev)
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, 4))[0].to(dev)
    gen = torch.Generator().manual_seed(44)
    target, target_depth = torch.rand((3, H, W), generator=gen).to(dev), (1.0 + 3.0 * torch.rand((H, W), generator=gen)).to(dev)
    routes, held = {}, {}
    for route in ("torch", "fused"):
        params = {k: torch.nn.Parameter(v.to(dev).requires_grad_(True)) for k, v in init.items()}
        groups = [{"params": [v], "name": k, "lr": LRS["mapping"][k]} for k, v in params.items()]
        opt = torch.optim.Adam(groups, lr=0.0, eps=1e-15) if route == "torch" else FusedAdam(groups, lr=0.0, eps=1e-15)
        held[route] = (params, opt)

        def step(params=params, opt=opt):
            pts = params["means3D"]
            tp = (w2c @ torch.cat((pts, torch.ones_like(pts[:, :1])), 1).T).T[:, :3]
            im, radius, depth_sil, rv = render_rgb_depth_sil(params, cam, w2c, tp)
            loss = 0.5 * (im - target).abs().mean() + (depth_sil[0] - target_depth).abs().mean()
            loss.backward()
            opt.step()
            opt.zero_grad(set_to_none=True)

        routes[route] = step
    res = compare(routes, 10)
    for k in ("torch", "fused"):
        e, w = res[k]["event_ms"], res[k]["wall_ms"]
        lines.append(f"mapping iteration P={P} {W}x{H}  optimizer {k:5s}  event {e['median']:.3f} ms [{e['min']:.3f} .. {e['max']:.3f}]   "
                     f"wall {w['median']:.3f} ms [{w['min']:.3f} .. {w['max']:.3f}]")
    res["saved_event_ms"] = res["torch"]["event_ms"]["median"] - res["fused"]["event_ms"]["median"]
    lines.append(f"mapping iteration P={P} {W}x{H}  torch - fused = {res['saved_event_ms']:.3f} ms per iteration (event)")
    return res


if "--kernels-only" in sys.argv:
    route, config, iters, P = _opt("--kernels-only"), _opt("--config", "mapping"), int(_opt("--iters", "10")), int(_opt("--size", "20000"))
    opt, _ = make(P, config, route)
    for _ in range(iters):
        opt.step()
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, config=config, iters=iters, size=P)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]


def save():
    if args:
        with open(args[0], "w") as f:
            json.dump(out, f, indent=1)
        with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
            f.write("\n".join(lines) + "\n")


sizes = [int(s) for s in _opt("--sizes", "20000,2000000").split(",")]
out = dict(what="optimizer.step() of the reference's mapping and tracking optimizers: torch.optim.Adam against FusedAdam (and FusedAdam(skip_frozen=True) "
                "in tracking); ms per step, median [min .. max] of 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, cases={})
lines = []
for P in sizes:
    iters = 200 if P <= 100000 else 20
    for config, names in ROUTES.items():
        made = {r: make(P, config, r) for r in names}
        res = compare({r: made[r][0].step for r in names}, iters)
        res["iters"] = iters
        res["host_syncs"] = {r: host_syncs(made[r][0].step) for r in names}
        for r in names:
            res[r]["elements"] = made[r][1]
            res[r]["bytes_per_s"] = 28.0 * made[r][1] / (res[r]["event_ms"]["median"] * 1e-3)
            e, w = res[r]["event_ms"], res[r]["wall_ms"]
            lines.append(f"{config:8s} P={P}  {r:10s}  event {e['median']:.4f} ms [{e['min']:.4f} .. {e['max']:.4f}]   wall {w['median']:.4f} ms "
                         f"[{w['min']:.4f} .. {w['max']:.4f}]   host syncs {res['host_syncs'][r]}   {made[r][1]} elements, "
                         f"{res[r]['bytes_per_s'] / 1e12:.3f} TB/s at 28 B/element ({100 * res[r]['bytes_per_s'] / COPY_RATE:.1f} % of the 6.29 TB/s copy rate)")
        for r in names[1:]:
            for what in ("event_ms", "wall_ms"):
                res[f"torch_over_{r}_{what}"] = res["torch"][what]["median"] / res[r][what]["median"]
                res[f"{r}_range_below_torch_range_{what}"] = res[r][what]["max"] < res["torch"][what]["min"]
            lines.append(f"{config:8s} P={P}  torch / {r} = {res[f'torch_over_{r}_event_ms']:.2f}x (event), {res[f'torch_over_{r}_wall_ms']:.2f}x (wall); "
                         f"whole range below torch's: {res[f'{r}_range_below_torch_range_event_ms']}")
        out["cases"][f"{config}/{P}"] = res
        del made
        torch.cuda.empty_cache()
if "--no-iteration" not in sys.argv:
    out["mapping_iteration"] = mapping_iteration(2_000_000, 512, 512, lines)
    torch.cuda.empty_cache()
save()                                   # the timings are on file before the traces start
if "--no-trace" not in sys.argv:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on the PATH: the launch counts cannot be traced (--no-trace leaves them out)")
    for config, names in ROUTES.items():
        n = out["cases"][f"{config}/{sizes[0]}"]["launches_per_step"] = {}
        for r in names:
            a, b = traced_kernels(r, config, 10, sizes[0]), traced_kernels(r, config, 20, sizes[0])
            n[r] = dict(all=(b[0] - a[0]) / 10.0, adam_kernels=(b[1] - a[1]) / 10.0)
        lines.append(f"launches per step, {config} P={sizes[0]} (kernel trace, runs of 10 and 20 steps, difference / 10): " +
                     ", ".join(f"{r} {n[r]['all']:.0f}" + (f" ({n[r]['adam_kernels']:.0f} k_adam_step)" if r != "torch" else "") for r in names))
    save()
print("\n".join(lines))
print(json.dumps(out))
