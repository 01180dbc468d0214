#!/usr/bin/env python3
"""tools/render_eval_bench.py [out.txt] | --count ROUTE N: what the render-quality evaluation of a map costs (GaussianSLAM.eval_views ->
fr_render_views + fr_view_metrics) on the benchmark map of BASELINE.json configs[1] (500k Gaussians, 256 x 256, seed 2), against what
a caller had before it.  Route A is measured on its own code, never on the new call:
  A1  the reference's calling pattern: per pose render_at_pose, clamp, calc_psnr(...).mean() (the reference's two torch lines),
      mean |depth - depth_gt|, the product's calc_ssim (the image-loss kernel), the isinf skip and four .item() reads
  A2  one render_at_poses call, then the same metric chain and reads per view
  B   eval_views: 64 views with float targets in one chunk; 2000 views with uint8 RGBA targets in chunks of 64
All routes alternate in one process, 7 repeats after a warm-up, a host clock around a final device synchronise and a pair of
device events around the same work; median [min .. max].  The spread is max / min over a route's own repeats (identical runs).
The metric launches alone (ops.view_metrics, 64 views, float targets, depth) are timed with device events over 50 calls and set
against the bytes they must move -- render, target, depth and depth target once each -- at the 6.3 TB/s copy rate README.md quotes.

`--count ROUTE N` (ROUTE: A1, A2, B64; a run of its own, under `rocprofv3 --kernel-trace --stats`): a warm-up, then N evaluations
of 64 views with torch's sync debug mode counting the host reads; two such runs with different N give the launches per evaluation
as a difference, free of the scene's one-off kernels."""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from fisher_rast import ops, synthetic                                   # noqa: E402
from models.SLAM.gaussian import GaussianSLAM                            # noqa: E402
from models.SLAM.utils.slam_external import calc_ssim                    # noqa: E402

dev = torch.device("cuda:0")
P, W, SEED, V, VBIG, CHUNK, REPS = 500_000, 256, 2, 64, 2000, 64, 7
COPY_RATE = 6.3e12                                                       # B/s, README.md (4.86 TB/s is 77 % of it)
slam = GaussianSLAM(params=synthetic.room_shell(P, SEED), intrinsics=synthetic.intrinsics(W, W), width=W, height=W, device=dev)


def targets(c2w, seed):
    """ground truth for poses: the map's own clamped render plus noise as bytes [n,W,W,4] (the fourth channel random), and its depth
    plus noise -- made chunk by chunk"""
    g = torch.Generator(device=dev).manual_seed(seed)
    rgba, depth = [], []
    for v0 in range(0, c2w.shape[0], CHUNK):
        r = slam.render_at_poses(c2w[v0:v0 + CHUNK])
        n = r["render"].shape[0]
        x = (r["render"].clamp(0.0, 1.0) + 0.05 * torch.randn(r["render"].shape, generator=g, device=dev)).clamp(0.0, 1.0)
        a = torch.randint(0, 256, (n, W, W, 1), generator=g, device=dev, dtype=torch.uint8)
        rgba.append(torch.cat((torch.round(x * 255).to(torch.uint8).permute(0, 2, 3, 1), a), dim=-1).contiguous())
        depth.append((r["depth"] + 0.05 * torch.randn(r["depth"].shape, generator=g, device=dev)).clamp_min(0.0))
    return torch.cat(rgba), torch.cat(depth)


c2w = synthetic.candidate_poses(V, SEED).to(dev).float()
rgba, depth_gt = targets(c2w, 1)
rgb_gt = (rgba[..., :3].permute(0, 3, 1, 2) / 255).contiguous()


def chain(color, depth, gt, dgt, metrics):
    """eval_navigation's lines 1451-1491 for one pose, LPIPS left out: four host reads"""
    color = color.detach().clamp_(min=0., max=1.)
    mse = ((color - gt) ** 2).view(3, -1).mean(1, keepdim=True)
    psnr = (20 * torch.log10(1.0 / torch.sqrt(mse))).mean()
    depth_mae = torch.mean(torch.abs(depth.detach() - dgt))
    stat = psnr.item()                                               # poses_stats
    ssim_score = calc_ssim(color.unsqueeze(0), gt.unsqueeze(0))
    if stat == float("inf") or stat == float("-inf"):
        return
    metrics["psnr"].append(psnr.item())
    metrics["depth_mae"].append(depth_mae.item())
    metrics["ssim"].append(ssim_score.item())


def route_a1():
    m = dict(psnr=[], depth_mae=[], ssim=[])
    for v in range(V):
        pkg = slam.render_at_pose(c2w[v])
        chain(pkg["render"], pkg["depth"], rgb_gt[v], depth_gt[v], m)
    return {k: sum(x) / len(x) for k, x in m.items()}


def route_a2():
    m = dict(psnr=[], depth_mae=[], ssim=[])
    r = slam.render_at_poses(c2w)
    for v in range(V):
        chain(r["render"][v], r["depth"][v], rgb_gt[v], depth_gt[v], m)
    return {k: sum(x) / len(x) for k, x in m.items()}


def route_b64():
    return slam.eval_views(c2w, rgb_gt, depth_gt, chunk=CHUNK).mean


def timed(fn):
    """(host ms around a final synchronise, device ms between two events)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)


if "--count" in sys.argv:
    name, n = sys.argv[sys.argv.index("--count") + 1], int(sys.argv[sys.argv.index("--count") + 2])
    fn = dict(A1=route_a1, A2=route_a2, B64=route_b64)[name]
    fn()
    fn()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        for _ in range(n):
            fn()
    torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    print(json.dumps(dict(route=name, evaluations=n, views=V, host_reads_per_evaluation=len(caught) / n, host_reads_per_view=len(caught) / n / V)))
    sys.exit(0)

c2w_big = synthetic.candidate_poses(VBIG, SEED + 1).to(dev).float()
rgba_big, depth_big = targets(c2w_big, 2)


def route_b2000():
    return slam.eval_views(c2w_big, rgba_big, depth_big, chunk=CHUNK).mean


fns = dict(A1_loop_render_at_pose=route_a1, A2_render_at_poses_then_chain=route_a2, B_eval_views_64_f32=route_b64, B_eval_views_2000_u8=route_b2000)
views = dict(A1_loop_render_at_pose=V, A2_render_at_poses_then_chain=V, B_eval_views_64_f32=V, B_eval_views_2000_u8=VBIG)
means = {}
for k, fn in fns.items():                                     # warm-up: workspaces, capacity hints, the allocator
    fn()
    means[k] = fn()
ms = {k: [] for k in fns}
for _ in range(REPS):                                         # alternating: every repeat runs all routes
    for k, fn in fns.items():
        ms[k].append(timed(fn))


def stat(v):
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


lines = [f"render-quality evaluation on BASELINE.json configs[1] ({P} Gaussians, {W}x{W}, seed {SEED}) on {torch.cuda.get_device_name(0)}: "
         f"{REPS} alternating repeats after warm-up; host ms around a final synchronise | device ms between events; median [min .. max]"]
res = {}
for k in fns:
    h, d = stat([a for a, _ in ms[k]]), stat([b for _, b in ms[k]])
    res[k] = dict(host=h, device=d, spread=h[2] / h[1], us_per_view=1e3 * h[0] / views[k])
    lines.append(f"{k:30s} {views[k]:5d} views  host {h[0]:9.3f} [{h[1]:.3f} .. {h[2]:.3f}]  device {d[0]:9.3f} [{d[1]:.3f} .. {d[2]:.3f}] ms  "
                 f"{res[k]['us_per_view']:8.1f} us/view  spread (max/min) {res[k]['spread']:.3f}")
a1, a2, b, bb = (res[k] for k in fns)
spread = max(a2["spread"], b["spread"])
ratio = a2["host"][0] / b["host"][0]
lines.append(f"A2 / B(64) = {ratio:.2f}x (medians), A1 / B(64) = {a1['host'][0] / b['host'][0]:.2f}x; run-to-run spread of identical runs "
             f"{spread:.3f}x (the larger of A2's and B's max/min); B's slowest run {b['host'][2]:.3f} ms against A2's fastest {a2['host'][1]:.3f} ms: "
             + ("B is faster than A2 by more than the spread" if ratio > spread and b["host"][2] < a2["host"][1] else
                "the ratio does NOT exceed the spread: no speed-up is claimed"))
lines.append(f"per view: A2 {a2['us_per_view']:.1f} us, B(64, f32) {b['us_per_view']:.1f} us, B(2000, u8 RGBA, chunks of {CHUNK}) {bb['us_per_view']:.1f} us")
lines.append("means (psnr, ssim, depth_mae): " + "; ".join(f"{k.split('_')[0]} " + " ".join(f"{means[k][n]:.6f}" for n in ("psnr", "ssim", "depth_mae"))
                                                              for k in list(fns)[:3]))

# the metric launches alone, 64 views
r = slam.render_at_poses(c2w)
render, depth = r["render"], r["depth"]
for _ in range(5):
    ops.view_metrics(render, rgb_gt, depth, depth_gt)
e = [torch.cuda.Event(enable_timing=True) for _ in range(51)]
torch.cuda.synchronize()
e[0].record()
for i in range(50):
    ops.view_metrics(render, rgb_gt, depth, depth_gt)
    e[i + 1].record()
torch.cuda.synchronize()
us = sorted(1e3 * e[i].elapsed_time(e[i + 1]) for i in range(50))
nbytes = V * W * W * 4 * (3 + 3 + 1 + 1)
bound_us = 1e6 * nbytes / COPY_RATE
lines.append(f"metric launches alone (fr_view_metrics: tiles, rows, summary), {V} views f32 + depth: {us[25]:.1f} us [{us[0]:.1f} .. {us[-1]:.1f}] per call "
             f"(device events, 50 calls); bytes that must move {nbytes / 1e6:.1f} MB = {bound_us:.1f} us at {COPY_RATE / 1e12:.1f} TB/s: "
             f"the bandwidth bound is {100 * bound_us / us[25]:.0f} % of the measured time")
print("\n".join(lines))
args = [a for a in sys.argv[1:] if not a.startswith("--")]
if args:
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
