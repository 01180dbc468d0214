#!/usr/bin/env python3
"""tools/point_scores_bench.py [out.json] [--kernels-only [--columns C]]: cost of the candidate scan's per-Gaussian scores -- the
running maximum over 64 candidate views of point[v, i] = sum_c cur_H[v, i, c] H_inv[i, c] -- on the benchmark map of BASELINE.json
configs[1] (500k Gaussians, 256 x 256, seed 2) with its 64 candidate poses, for 4 and 11 Fisher columns:
  fused      FisherScorer.point_scores(per_view=False) -> fr_fisher_point_views: one accumulator per (view, Gaussian)
  per_view   distributed.sharded_point_score_max at world size 1, the route a caller had before: out_H per view for 16 views at a
             time into a [16, P, C] tensor, contracted with H_inv and reduced in torch
  fused_16   the fused route in four calls of 16 views into one running maximum: the per-view route's granularity, hence a workspace
             (key segments, records, lists) for 16 views instead of 64 -- the like-for-like memory figure
All in one process, 7 alternating repeats after a warm-up, the whole call, a host clock around a device synchronise; median
[min .. max].  Peak device memory above the map (scorer, H_inv and map tensors allocated; a fresh scorer per route, so the route's
own workspaces count) is recorded for each.  The kernel table comes from a run of its own:
  rocprofv3 --kernel-trace --stats -d <dir> -o stats --output-format csv -- python3 tools/point_scores_bench.py --kernels-only --columns 4
(`--kernels-only`: a warm-up and 10 fused calls, nothing else, for the trace).  The share of the global float atomics in
k_fisher_point_tile: tools/fe_ablate.py --point."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from fisher_rast import synthetic, distributed      # noqa: E402
from fisher_rast.ops import FisherScorer            # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera   # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--") and not a.isdigit()]
kernels_only = "--kernels-only" in sys.argv
only_columns = int(sys.argv[sys.argv.index("--columns") + 1]) if "--columns" in sys.argv else None
dev = torch.device("cuda:0")
P, W, SEED, V, KF, REPS = 500_000, 256, 2, 64, 16, 7
act = {k: v.to(dev) for k, v in synthetic.activate(synthetic.room_shell(P, SEED)).items()}
cam = setup_camera(W, W, synthetic.intrinsics(W, W), np.eye(4), device=dev)
w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, SEED)).to(dev)
kf = synthetic.invert_rigid(synthetic.candidate_poses(KF, 102)).to(dev)


def scorer(C):
    return FisherScorer(cam, *(act[k] for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")), columns=C)


def h_inv(sc):
    Ht = torch.zeros((P, sc.columns), device=dev)
    sc.run(kf, out_H=Ht)
    return torch.reciprocal(Ht + 0.1)


def fused(sc, Hi):
    return sc.point_scores(w2c, Hi, per_view=False)["point_max"]


def per_view(sc, Hi):
    return distributed.sharded_point_score_max(sc, w2c, Hi)


def fused_16(sc, Hi):
    """the fused route at the per-view route's granularity: 16 views per call into one running maximum (a workspace for 16 views)"""
    best = torch.zeros((P,), device=dev)
    for v0 in range(0, V, 16):
        sc.point_scores(w2c[v0:v0 + 16], Hi, per_view=False, point_max=best)
    return best


def once(fn, *a):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn(*a)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


if kernels_only:
    sc = scorer(only_columns or 4)
    Hi = h_inv(sc)
    fused(sc, Hi)
    torch.cuda.synchronize()
    for _ in range(10):
        fused(sc, Hi)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=True, calls=10, views=V, columns=sc.columns)))
    sys.exit(0)

fns = dict(fused=fused, per_view=per_view, fused_16=fused_16)
out = dict(what="running maximum over 64 candidate views of the per-Gaussian scores on BASELINE.json configs[1] (500k Gaussians, 256x256, "
                "seed 2): ms per 64 views (whole call), host clock around a device synchronise, 7 alternating repeats after warm-up; "
                "peak device memory of one call above the map, MB",
           device=torch.cuda.get_device_name(0), views=V, repeats=REPS, columns={})
lines = []
for C in ([only_columns] if only_columns else [4, 11]):
    sc = scorer(C)
    Hi = h_inv(sc)
    for fn in fns.values():                                   # warm-up: workspaces, capacity hints, the allocator
        fn(sc, Hi)
        fn(sc, Hi)
    ms = {k: [] for k in fns}
    for _ in range(REPS):                                     # alternating: every repeat runs all three
        for k, fn in fns.items():
            ms[k].append(once(fn, sc, Hi))
    a, b = fused(sc, Hi), per_view(sc, Hi)
    rel = float((a - b).abs().max() / b.abs().max())
    rows = {}
    for k, v in ms.items():
        v = sorted(v)
        rows[k] = dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], ms_all=ms[k])
    del sc, a, b
    # peak memory above the map: a fresh scorer per route (its workspaces are the route's), H_inv allocated
    for k, fn in fns.items():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        s2 = scorer(C)
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn(s2, Hi)
        torch.cuda.synchronize()
        rows[k]["peak_mb_above_map"] = (torch.cuda.max_memory_allocated() - base) / 1e6
        del s2
    res = dict(rows=rows, fused_range_below_per_view_range=rows["fused"]["ms_max"] < rows["per_view"]["ms_min"],
               ratio_per_view_over_fused=rows["per_view"]["ms_median"] / rows["fused"]["ms_median"], max_rel_diff_of_the_maxima=rel)
    out["columns"][str(C)] = res
    for k, r_ in rows.items():
        lines.append(f"columns {C:2d}  {k:9s} {r_['ms_median']:9.3f} ms  [{r_['ms_min']:.3f} .. {r_['ms_max']:.3f}]   peak {r_['peak_mb_above_map']:8.1f} MB above the map")
    lines.append(f"columns {C:2d}  per_view / fused = {res['ratio_per_view_over_fused']:.2f}x; fused range entirely below the per-view route's: "
                 f"{res['fused_range_below_per_view_range']}; max |difference| of the two maxima / largest = {rel:.2e}")
    del Hi
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
