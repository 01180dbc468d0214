#!/usr/bin/env python3
"""tools/render_views_bench.py [out.json] [--kernels-only]: cost of rendering a batch of candidate poses
(GaussianSLAM.render_at_poses -> FisherScorer.render_views -> fr_render_views) on the benchmark map of BASELINE.json configs[1]
(500k Gaussians, 256 x 256, seed 2) with its 64 candidate poses, against what a caller had before:
  loop_render_at_pose   64 x GaussianSLAM.render_at_pose (torch matmul + two single-view rasteriser calls per pose)
  loop_forward_pair     64 x render_rgb_depth_sil (one single-view forward_pair per pose: one projection / binning / sort, two images)
All three in one process, 7 alternating repeats after a warm-up, a host clock around a device synchronise; median [min .. max].
The tile kernel's algorithmic traffic -- (8 + 48) B per listed tile instance (key + render record) plus the written pixels -- is
reported per call; divide by the kernel's own time from
  rocprofv3 --kernel-trace --stats -d <dir> -o stats --output-format csv -- python3 tools/render_views_bench.py --kernels-only
(`--kernels-only`: a warm-up and 10 batched calls, nothing else, for the trace)."""
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
from fisher_rast import synthetic                                       # noqa: E402
from models.SLAM.gaussian import GaussianSLAM                            # noqa: E402
from models.SLAM.utils.slam_helpers import render_rgb_depth_sil          # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
kernels_only = "--kernels-only" in sys.argv
dev = torch.device("cuda:0")
P, W, SEED, V, REPS = 500_000, 256, 2, 64, 7
slam = GaussianSLAM(params=synthetic.room_shell(P, SEED), intrinsics=synthetic.intrinsics(W, W), width=W, height=W, device=dev)
c2w = synthetic.candidate_poses(V, SEED).to(dev).float()
w2c = synthetic.invert_rigid(c2w.cpu()).to(dev)
eye = torch.eye(4, device=dev)


def batched():
    return slam.render_at_poses(c2w)


def loop_render_at_pose():
    return [slam.render_at_pose(c) for c in c2w]


def loop_forward_pair():
    x, y, z = (slam.params["means3D"][:, k] for k in range(3))
    out = []
    for w in w2c:
        m = torch.stack([((x * w[r, 0] + y * w[r, 1]) + z * w[r, 2]) + w[r, 3] for r in range(3)], dim=1)
        im, _, depth_sil, _ = render_rgb_depth_sil(slam.params, slam.cam, eye, m)
        out.append((im.detach(), depth_sil.detach()))
    return out


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


if kernels_only:
    batched()
    torch.cuda.synchronize()
    for _ in range(10):
        batched()
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=True, calls=10, views=V)))
    sys.exit(0)

fns = dict(render_at_poses=batched, loop_render_at_pose=loop_render_at_pose, loop_forward_pair=loop_forward_pair)
for fn in fns.values():                                   # warm-up: workspaces, capacity hints, the allocator
    fn()
    fn()
ms = {k: [] for k in fns}
for _ in range(REPS):                                     # alternating: every repeat runs all three
    for k, fn in fns.items():
        ms[k].append(once(fn))

# same images: the batch against the forward_pair loop fed with the library's own inverse (bit for bit: tests/test_gpu_render_views.py);
# here a coarse check that the three routes render the same thing
b = batched()
l = loop_render_at_pose()
diff = max(float((b["render"][v] - l[v]["render"].detach()).abs().max()) for v in range(V))
ddiff = max(float((b["depth"][v] - l[v]["depth"].detach()).abs().max()) for v in range(V))

# algorithmic bytes of the tile kernel per call
sc = slam._scorer()
r = sc.render_launch(w2c, depth=False, final_T=False)
torch.cuda.synchronize()
listed = int(r["status"].cpu()[0])
pix_bytes = V * 6 * W * W * 4
tile_bytes = listed * (8 + 48) + pix_bytes

rows = {}
for k, v in ms.items():
    v = sorted(v)
    rows[k] = dict(ms_median=v[len(v) // 2], ms_min=v[0], ms_max=v[-1], views_per_s=1e3 * V / v[len(v) // 2], ms_all=ms[k])
out = dict(what="render of 64 candidate poses (RGB + depth + silhouette) on BASELINE.json configs[1] (500k Gaussians, 256x256, seed 2): "
                "ms per 64 poses, host clock around a device synchronise, 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), views=V, repeats=REPS, rows=rows,
           batched_range_below_loop_range=rows["render_at_poses"]["ms_max"] < rows["loop_render_at_pose"]["ms_min"],
           ratio_loop_render_at_pose_over_batched=rows["loop_render_at_pose"]["ms_median"] / rows["render_at_poses"]["ms_median"],
           ratio_loop_forward_pair_over_batched=rows["loop_forward_pair"]["ms_median"] / rows["render_at_poses"]["ms_median"],
           max_abs_diff_vs_render_at_pose=dict(render=diff, depth=ddiff),
           tile_kernel=dict(listed_tile_instances=listed, visible=int(r["vis_count"].sum()), rectangle_instances=int(r["num_rendered"].sum()),
                            bytes_keys_and_records=listed * 56, bytes_pixels=pix_bytes, algorithmic_bytes=tile_bytes,
                            note="divide by k_render_views_tile<6>'s time of the rocprofv3 --kernel-trace --stats run"))
lines = [f"{k:22s} {r_['ms_median']:9.3f} ms  [{r_['ms_min']:.3f} .. {r_['ms_max']:.3f}]  {r_['views_per_s']:9.0f} views/s" for k, r_ in rows.items()]
lines.append(f"loop_render_at_pose / render_at_poses = {out['ratio_loop_render_at_pose_over_batched']:.2f}x, "
             f"loop_forward_pair / render_at_poses = {out['ratio_loop_forward_pair_over_batched']:.2f}x; "
             f"batched range entirely below the render_at_pose loop's: {out['batched_range_below_loop_range']}")
lines.append(f"tile kernel: {listed} listed tile instances x 56 B + {pix_bytes} B of pixels = {tile_bytes / 1e6:.1f} MB per call; "
             f"max |diff| against render_at_pose: render {diff:.2e}, depth {ddiff:.2e}")
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
