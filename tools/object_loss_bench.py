#!/usr/bin/env python3
"""tools/object_loss_bench.py [out.txt] [--sizes 20000,2000000] [--images 256,512] [--no-launches]

What the object-aware training step costs: one `get_loss` + `backward` of make_get_loss(object_mask=True) through the fused render
pair and the fused loss terms, with an object mask over about half of the frame, on a map of 20k and of 2M Gaussians at 256 x 256
and 512 x 512, in tracking and in mapping, with and without ignore_outlier_depth_loss:
  torch   fused_mask=False: the pixel mask is the chain of comparisons, isnan calls and ANDs (with a Tensor.median() when outliers
          are rejected), the object lines are the reference's torch lines and autograd
  fused   fused_mask=True: fr_loss_mask and fr_bg_penalty_forward / _backward
Both routes run in this process, alternating: ITERS calls between two device events, REPS repeats after a warm-up; median
[min .. max] -- the range is the spread of identical runs.  Launches per call are the device kernels torch's profiler records during
one call (memsets and copies apart); host synchronisations are what torch's sync debug mode reports during one call.

Then `get_gaussians_outside_mask` (models/SLAM/utils/slam_external.py: fr_outside_mask, one host read) against the reference's torch
chain (two nonzero calls, four .item() reads) at the same map sizes, 512 x 512 mask; wall ms, since both end on the host.

Writes profiles/object_loss_bench.txt (or the path given)."""
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from fisher_rast import synthetic                                   # noqa: E402
from models.SLAM.gaussian import make_get_loss                      # noqa: E402
from models.SLAM.utils import slam_external as se                   # noqa: E402
from models.SLAM.utils import slam_helpers as sh                    # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera            # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS = 7
lines = []


def say(line):
    print(line, flush=True)
    lines.append(line)


def timed(step, iters, wall=False):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / iters if wall else e0.elapsed_time(e1) / iters


def compare(routes, iters, wall=False):
    for step in routes.values():
        for _ in range(3):
            step()
    raw = {k: [] for k in routes}
    for _ in range(REPS):
        for k, step in routes.items():
            raw[k].append(timed(step, iters, wall))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in raw.items()}


def host_syncs(step):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


def launches(step):
    """device kernels during one call, by torch's profiler; None where it records none"""
    if "--no-launches" in sys.argv:
        return None
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and not any(w in e.name.lower() for w in ("memset", "memcpy")))
    return n or None


def verdict(res):
    (tm, tlo, thi), (fm, flo, fhi) = res["torch"], res["fused"]
    spread = max(thi - tlo, fhi - flo)
    return f"torch / fused = {tm / fm:.2f}x; fused - torch = {fm - tm:+.4f} ms, spread of identical runs {spread:.4f} ms: " + \
           ("fused is SLOWER than torch by more than the spread" if fm - tm > spread else "fused is not slower")


def object_step(P, size, tracking, ignore):
    W = H = size
    init = {k: v.contiguous() for k, v in synthetic.room_shell(P, 4).items()}
    init["cam_unnorm_rots"] = torch.tensor([[[1.0], [0.0], [0.0], [0.0]]])
    init["cam_trans"] = torch.zeros((1, 3, 1))
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=dev)
    gen = torch.Generator().manual_seed(44)
    obj = torch.zeros((H, W), dtype=torch.bool)
    obj[H // 8: H - H // 8, W // 6: W - W // 6] = True
    curr = dict(cam=cam, w2c=torch.eye(4, device=dev), im=torch.rand((3, H, W), generator=gen).to(dev),
                depth=(1.0 + 3.0 * torch.rand((1, H, W), generator=gen)).to(dev), obj_mask_2d=obj.to(dev))
    weights = dict(im=0.5, depth=1.0)
    routes = {}
    for route in ("torch", "fused"):
        params = {k: v.to(dev).requires_grad_(True) for k, v in init.items()}
        variables = dict(max_2D_radius=torch.zeros(P, device=dev), means2D_gradient_accum=torch.zeros(P, device=dev), denom=torch.zeros(P, device=dev))
        get_loss = make_get_loss(sh.transform_to_frame, sh.calc_loss if tracking else sh.calc_loss_mask, fused_rendervar=True, object_mask=True,
                                 fused_mask=(route == "fused"))

        def step(params=params, variables=variables, get_loss=get_loss):
            loss, _, _ = get_loss(params, curr, variables, 0, weights, True, 0.5, True, ignore, tracking=tracking, mapping=not tracking)
            loss.backward()
            for v in params.values():
                v.grad = None

        routes[route] = step
    res = compare(routes, 20 if P <= 100000 else 10)
    tag = f"{'tracking' if tracking else 'mapping '} P={P:<8d} {W}x{H} ignore_outlier_depth_loss={int(ignore)}"
    for k in ("torch", "fused"):
        n = launches(routes[k])
        say(f"{tag}  {k:5s}  {res[k][0]:.4f} ms [{res[k][1]:.4f} .. {res[k][2]:.4f}]   launches {'not measured' if n is None else n}   "
            f"host syncs {host_syncs(routes[k])}")
    say(f"{tag}  {verdict(res)}")


def outside(P, size=512):
    g = torch.Generator().manual_seed(5)
    params = dict(means3D=(torch.rand((P, 3), generator=g) * 8 - 4).to(dev), log_scales=(torch.randn((P, 3), generator=g) - 3).to(dev),
                  cam_unnorm_rots=torch.tensor([[[0.9], [0.1], [-0.2], [0.3]]], device=dev), cam_trans=torch.tensor([[[0.3], [-0.2], [1.0]]], device=dev))
    f = float(size)
    curr = dict(id=0, intrinsics=torch.tensor([[f, 0, size / 2], [0, f, size / 2], [0, 0, 1]], device=dev))
    obj = torch.zeros((size, size), dtype=torch.bool, device=dev)
    obj[size // 8: size - size // 8, size // 6: size - size // 6] = True

    def torch_chain():
        """the reference's get_gaussians_outside_mask (slam_external.py:270-343), op for op"""
        from models.SLAM.gaussian import frame_w2c
        w2c = frame_w2c(params, 0)
        means = params['means3D']
        cam = (w2c[:3, :3] @ means.T + w2c[:3, 3:4]).T
        z = cam[:, 2]
        p = (curr['intrinsics'] @ cam.T).T
        u, v = p[:, 0] / p[:, 2].clamp_min(1e-6), p[:, 1] / p[:, 2].clamp_min(1e-6)
        in_img = (z > 0) & (u >= 0) & (u < size) & (v >= 0) & (v < size)
        iu, iv = u[in_img].round().long().clamp(0, size - 1), v[in_img].round().long().clamp(0, size - 1)
        inside = torch.zeros(means.shape[0], dtype=torch.bool, device=dev)
        inside[in_img] = obj[iv, iu]
        out = ~inside
        scale_max = torch.exp(params['log_scales']).max(dim=1).values
        idx_in, idx_out = torch.nonzero(inside).squeeze(1), torch.nonzero(out).squeeze(1)
        rng = lambda x: (float('nan'), float('nan')) if x.numel() == 0 else (x.min().item(), x.max().item())
        return out, rng(scale_max[idx_in]) + rng(scale_max[idx_out])

    routes = dict(torch=torch_chain, fused=lambda: se.get_gaussians_outside_mask(params, curr, obj, with_indices=False),
                  fused_idx=lambda: se.get_gaussians_outside_mask(params, curr, obj))
    res = compare(routes, 10, wall=True)
    for k, name in (("torch", "torch chain"), ("fused", "library, with_indices=False"), ("fused_idx", "library, with the index lists")):
        n = launches(routes[k])
        say(f"outside mask P={P:<8d} {size}x{size}  {name:30s} wall {res[k][0]:.4f} ms [{res[k][1]:.4f} .. {res[k][2]:.4f}]   "
            f"launches {'not measured' if n is None else n}   host syncs {host_syncs(routes[k])}")
    say(f"outside mask P={P:<8d} {verdict(dict(torch=res['torch'], fused=res['fused_idx']))}")


sizes = [int(s) for s in _opt("--sizes", "20000,2000000").split(",")]
images = [int(s) for s in _opt("--images", "256,512").split(",")]
target = next((a for a in sys.argv[1:] if a.endswith(".txt")), os.path.join(ROOT, "profiles", "object_loss_bench.txt"))
say(f"object-aware get_loss + backward, torch route (fused_mask=False) against fused (fused_mask=True), on {torch.cuda.get_device_name(0)}: "
    f"event ms per call, median [min .. max] of {REPS} alternating repeats")
for P in sizes:
    for size in images:
        for tracking in (True, False):
            for ignore in (False, True):
                object_step(P, size, tracking, ignore)
                torch.cuda.empty_cache()
for P in sizes:
    outside(P)
with open(target, "w") as f:
    f.write("\n".join(lines) + "\n")
