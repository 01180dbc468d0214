#!/usr/bin/env python3
"""tools/pose_fisher_bench.py [out.json]: cost of the camera-pose Fisher information (FisherScorer.pose_fisher, fr_fisher_pose_views)
on the benchmark map of BASELINE.json configs[1] (500k Gaussians, 256 x 256, seed 2): ms per call and us per view for 64 views and for
630 views (21 paths x 30 steps of the planner, split by the launch limit), next to the scorer's 64-view score-only launch.
Wall time per call (each call ends with the status read, as the planner's does), and the pose kernel's own time from the library's
event pair (fr_profile_enable)."""
import ctypes
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
from fisher_rast import _lib, synthetic                      # noqa: E402
from fisher_rast.ops import FisherScorer                     # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera     # noqa: E402

dev = torch.device("cuda:0")
P, W, SEED = 500_000, 256, 2
act = {k: v.to(dev) for k, v in synthetic.activate(synthetic.room_shell(P, SEED)).items()}
cam = setup_camera(W, W, synthetic.intrinsics(W, W), np.eye(4), device=dev)
sc = FisherScorer(cam, act["means3D"], act["rgb_colors"], act["rotations"], act["opacities"], act["scales"])
v64 = synthetic.invert_rigid(synthetic.candidate_poses(64, SEED)).to(dev)
v630 = synthetic.invert_rigid(synthetic.candidate_poses(630, SEED + 1)).to(dev)
H_inv = torch.rand((P, 4), generator=torch.Generator().manual_seed(7)).to(dev) + 0.05
lib = _lib.load()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def kernel_ms(fn, reps):
    """mean of the library's per-launch event durations (the dominant kernel of each fr_* call) over `reps` calls"""
    fn()
    torch.cuda.synchronize()
    lib.fr_profile_enable(1)
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    buf = (ctypes.c_float * 4096)()
    n = lib.fr_profile_fetch(buf, 4096)
    lib.fr_profile_enable(0)
    return float(np.sum(buf[:n])) / reps, n // reps


rows = {}
ms = timed(lambda: sc.run(v64, H_inv=H_inv)["scores"], 20)
k, _ = kernel_ms(lambda: sc.run(v64, H_inv=H_inv), 20)
rows["scorer_64"] = dict(views=64, ms_per_call=ms, us_per_view=1e3 * ms / 64, tile_kernel_ms=k, tile_kernel_us_per_view=1e3 * k / 64)
for name, w in (("pose_64", v64), ("pose_630", v630)):
    reps = 20 if w.shape[0] == 64 else 5
    ms = timed(lambda: sc.pose_fisher(w), reps)
    k, launches = kernel_ms(lambda: sc.pose_fisher(w), reps)
    V = int(w.shape[0])
    rows[name] = dict(views=V, ms_per_call=ms, us_per_view=1e3 * ms / V, tile_kernel_ms=k, tile_kernel_us_per_view=1e3 * k / V,
                      launches_per_call=launches)
H = sc.pose_fisher(v64)
ev = torch.linalg.eigvalsh(H.double())
rows["pose_64"]["checksum"] = float(H.double().sum())
rows["pose_64"]["smallest_eigenvalue_over_largest"] = float((ev[:, 0] / ev[:, -1]).min())
out = dict(what="camera-pose Fisher information on BASELINE.json configs[1] (500k Gaussians, 256x256, seed 2); "
                "ms per call = wall time incl. the status read; tile_kernel = k_fisher_pose_tile / k_fisher_tile_v4 events",
           device=torch.cuda.get_device_name(0), max_views_per_launch=sc.max_views_per_launch(), rows=rows)
for name, r in rows.items():
    print(f"{name:10s} {r['views']:4d} views  {r['ms_per_call']:8.3f} ms/call  {r['us_per_view']:7.2f} us/view  "
          f"(tile kernel {r['tile_kernel_ms']:.3f} ms, {r['tile_kernel_us_per_view']:.2f} us/view)")
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
