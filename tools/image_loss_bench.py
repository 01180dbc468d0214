#!/usr/bin/env python3
"""tools/image_loss_bench.py [out.json] [--P N] | --kernels-only fused|torch --iters K [--size S]

What the fused image loss (fr_image_loss_forward / _backward) costs against the torch chain it replaces:
  loss      one mapping-mode calc_loss, forward + backward, on a 3 x S x S render with its [1,S,S] depth, S = 256 and 512 (the
            image sizes of BASELINE.json configs[1] and configs[3]):
              fused   models/SLAM/utils/slam_helpers.calc_loss of this package (two launches forward, one backward per term)
              torch   the chain the caller handed to make_get_loss before: boolean-mask mean of |depth error|, 0.8 mean |.| +
                      0.2 (1 - ssim) with five grouped 11 x 11 conv2d -- written out below.  Its window is built ONCE here (the
                      reference rebuilds it on the host and copies it over in every call), which favours the torch side.
  get_loss  one mapping iteration of make_get_loss (fused render pair + loss + backward to the Gaussians) on the scene of
            tools/config4_train_step.py (2M Gaussians, 512 x 512, seed 4) with either loss.
Per route: ITERS iterations between two device events (event ms / iteration) and inside a host clock that ends in a device
synchronise (wall ms / iteration); REPS alternating repeats after a warm-up; median [min .. max].

Launch counts come from a kernel trace in runs of their own (tracing slows the host): per route
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/image_loss_bench.py --kernels-only fused --iters 10
and the same with --iters 20; (kernels in the second trace - kernels in the first) / 10 = launches per forward + backward."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import torch.nn.functional as F   # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from fisher_rast import synthetic                                   # noqa: E402
from models.SLAM.gaussian import make_get_loss                      # noqa: E402
from models.SLAM.utils import slam_helpers as sh                    # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera            # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, ITERS = 7, 500
TAPS = torch.tensor([np.exp(-(k - 5) ** 2 / 4.5) for k in range(11)], dtype=torch.float32)
TAPS = TAPS / TAPS.sum()
WINDOW = (TAPS[:, None] * TAPS[None, :]).expand(3, 1, 11, 11).contiguous().to(dev)


def torch_calc_loss(curr_data, im, depth, mask, color_mask, use_l1, use_sil_for_loss, ignore_outlier_depth_loss, tracking):
    """mapping mode of the chain this package's calc_loss replaces"""
    x, y = im, curr_data['im']
    blur = lambda a: F.conv2d(a[None], WINDOW, padding=5, groups=3)[0]
    mu1, mu2 = blur(x), blur(y)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    s1, s2, s12 = blur(x * x) - mu1_sq, blur(y * y) - mu2_sq, blur(x * y) - mu1_mu2
    ssim = ((2 * mu1_mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1_sq + mu2_sq + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
    return dict(depth=torch.abs(curr_data['depth'] - depth)[mask.detach()].mean(),
                im=0.8 * torch.abs(x - y).mean() + 0.2 * (1.0 - ssim.mean()))


def loss_inputs(S, seed=5):
    g = torch.Generator().manual_seed(seed)
    im = torch.rand((3, S, S), generator=g).to(dev).requires_grad_(True)
    depth = (torch.rand((1, S, S), generator=g) * 4 + 0.5).to(dev).requires_grad_(True)
    curr = dict(im=torch.rand((3, S, S), generator=g).to(dev), depth=(torch.rand((1, S, S), generator=g) * 4 + 0.5).to(dev))
    curr['depth'][0, :8, :] = 0.0
    mask = curr['depth'] > 0
    return curr, im, depth, mask, mask.repeat(3, 1, 1)


def loss_step(fn, inp):
    curr, im, depth, mask, cmask = inp
    im.grad = None
    depth.grad = None
    t = fn(curr, im, depth, mask, cmask, True, True, False, False)
    (0.5 * t['im'] + t['depth']).backward()
    return im.grad


def timed(step, iters):
    """(event ms, wall ms) per iteration of `iters` iterations"""
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
    """alternating repeats of every route; {name: {event: stats, wall: stats}}"""
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


if "--kernels-only" in sys.argv:
    route, iters, S = _opt("--kernels-only"), int(_opt("--iters", "10")), int(_opt("--size", "256"))
    inp = loss_inputs(S)
    fn = sh.calc_loss if route == "fused" else torch_calc_loss
    for _ in range(iters):
        loss_step(fn, inp)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, iters=iters, size=S)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]
out = dict(what="mapping-mode calc_loss forward + backward (3 x S x S render, [1,S,S] depth) and one make_get_loss mapping iteration, "
                "fused image loss against the torch chain; ms per iteration, median [min .. max] of 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, loss={}, get_loss={})
lines = []
for S in (256, 512):
    inp = loss_inputs(S)
    res = compare(dict(fused=lambda: loss_step(sh.calc_loss, inp), torch=lambda: loss_step(torch_calc_loss, inp)), ITERS)
    ga, gb = loss_step(sh.calc_loss, inp).clone(), loss_step(torch_calc_loss, inp).clone()
    res["max_rel_diff_of_the_image_gradients"] = float((ga - gb).abs().max() / gb.abs().max())
    for what in ("event_ms", "wall_ms"):
        res[f"torch_over_fused_{what}"] = res["torch"][what]["median"] / res["fused"][what]["median"]
        res[f"fused_range_below_torch_range_{what}"] = res["fused"][what]["max"] < res["torch"][what]["min"]
    out["loss"][str(S)] = res
    for k in ("fused", "torch"):
        e, w = res[k]["event_ms"], res[k]["wall_ms"]
        lines.append(f"calc_loss fwd+bwd 3x{S}x{S}  {k:5s}  event {e['median']:.4f} ms [{e['min']:.4f} .. {e['max']:.4f}]   "
                     f"wall {w['median']:.4f} ms [{w['min']:.4f} .. {w['max']:.4f}]")
    lines.append(f"calc_loss fwd+bwd 3x{S}x{S}  torch / fused = {res['torch_over_fused_event_ms']:.2f}x (event), "
                 f"{res['torch_over_fused_wall_ms']:.2f}x (wall); max |gradient difference| / largest = {res['max_rel_diff_of_the_image_gradients']:.2e}")

# ---- one mapping iteration of get_loss on the config-4 scene ------------------------------------------------------------------
P, S = int(_opt("--P", "2000000")), 512
base = {k: v.to(dev) for k, v in synthetic.room_shell(P, 4).items()}
params = {k: v.clone().requires_grad_(True) for k, v in base.items()}
cam = setup_camera(S, S, synthetic.intrinsics(S, S), np.eye(4), device=dev)
w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, 4))[0].to(dev)
g = torch.Generator().manual_seed(44)
curr_data = dict(cam=cam, w2c=torch.eye(4, device=dev), im=torch.rand((3, S, S), generator=g).to(dev),
                 depth=(torch.rand((1, S, S), generator=g) * 4 + 0.5).to(dev))
variables = dict(max_2D_radius=torch.zeros(P, device=dev), means2D_gradient_accum=torch.zeros(P, device=dev), denom=torch.zeros(P, device=dev))
weights = dict(im=0.5, depth=1.0)


def transform_to_frame(params, time_idx, gaussians_grad, camera_grad):
    pts = params['means3D'] if gaussians_grad else params['means3D'].detach()
    return (w2c @ torch.cat((pts, torch.ones_like(pts[:, :1])), 1).T).T[:, :3]


def iteration(get_loss):
    for v in params.values():
        v.grad = None
    loss, _, _ = get_loss(params, curr_data, variables, 0, weights, True, 0.5, True, False, mapping=True)
    loss.backward()
    return loss


routes = dict(fused=make_get_loss(transform_to_frame, sh.calc_loss), torch=make_get_loss(transform_to_frame, torch_calc_loss))
res = compare({k: (lambda gl=gl: iteration(gl)) for k, gl in routes.items()}, 5)
la, lb = float(iteration(routes["fused"]).detach()), float(iteration(routes["torch"]).detach())
res["loss_values"] = dict(fused=la, torch=lb)
for what in ("event_ms", "wall_ms"):
    res[f"torch_over_fused_{what}"] = res["torch"][what]["median"] / res["fused"][what]["median"]
    res[f"fused_range_below_torch_range_{what}"] = res["fused"][what]["max"] < res["torch"][what]["min"]
out["get_loss"] = dict(P=P, size=S, **res)
for k in ("fused", "torch"):
    e, w = res[k]["event_ms"], res[k]["wall_ms"]
    lines.append(f"get_loss iteration P={P} {S}x{S}  loss={k:5s}  event {e['median']:.3f} ms [{e['min']:.3f} .. {e['max']:.3f}]   "
                 f"wall {w['median']:.3f} ms [{w['min']:.3f} .. {w['max']:.3f}]")
lines.append(f"get_loss iteration  torch / fused = {res['torch_over_fused_event_ms']:.3f}x (event), {res['torch_over_fused_wall_ms']:.3f}x (wall); "
             f"loss {la:.6f} (fused) {lb:.6f} (torch)")
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
