#!/usr/bin/env python3
"""POp-GS block criteria (GaussianObjectSLAM.pose_eval_popgs_blocks): `fused=True` -- the block stage of fr_fisher_views, binary64
factorisations in registers -- against `fused=False`, the torch chain per pose (one more render, einsum, two isin, batched binary32
LAPACK, one float read back), in ONE process on ONE map and ONE set of probes: 64 poses, K = 6, 4 keyframes, a small map (room_shell
10k) and a large one (room_shell 500k, BASELINE.json configs[1]'s), 256 x 256.

The probes: `_draw_probes` is replaced by a hand-out of slices of one fixed tensor in call order, so both routes back-propagate the
same upstream images (keyframes first, then the poses, K at a time or all at once).  Every shape is warmed up first, the two routes
alternate, host clock around a synchronise.  Per route: median [min .. max], the kernels launched and the device-to-host copies of
one call (torch.profiler), and how far the float32 scores are apart.  Writes <out-dir>/popgs_block_bench.txt."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np      # noqa: E402
import torch            # noqa: E402
import __graft_entry__ as entry   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--maps", type=int, nargs="+", default=[10_000, 500_000])
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--poses", type=int, default=64)
ap.add_argument("--keyframes", type=int, default=4)
ap.add_argument("--K", type=int, default=6)
ap.add_argument("--lam", type=float, default=1e-6)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
args = ap.parse_args()

entry.build()
from fisher_rast import synthetic      # noqa: E402
import models.gaussian_slam as mgs     # noqa: E402

dev = torch.device("cuda:0")
S, V, K, F = args.size, args.poses, args.K, args.keyframes
lines, result = [], dict(config=dict(image=[S, S], poses=V, K=K, keyframes=F, lam=args.lam, reps=args.reps))


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), runs_ms=[round(x, 3) for x in ms])


def counted(fn):
    """(kernels launched, device-to-host copies) of one call, or (None, None) where the profiler gives no device events"""
    try:
        from torch.profiler import profile, ProfilerActivity
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        if not evs:
            return None, None
        d2h = sum(1 for e in evs if "memcpy" in e.name.lower() and ("dtoh" in e.name.lower() or "devicetohost" in e.name.lower().replace(" ", "")))
        kernels = sum(1 for e in evs if "memcpy" not in e.name.lower() and "memset" not in e.name.lower())
        return kernels, d2h
    except Exception as exc:                      # the numbers are a by-product: the timings stand without them
        say(f"  (profiler unavailable: {type(exc).__name__}: {exc})")
        return None, None


for P in args.maps:
    params = {k: v.to(dev) for k, v in synthetic.room_shell(P, 2).items()}
    slam = mgs.GaussianObjectSLAM(params=params, intrinsics=synthetic.intrinsics(S, S), width=S, height=S, device=dev)
    for kf in synthetic.invert_rigid(synthetic.candidate_poses(F, 102)):
        slam.add_keyframe(kf.to(dev))
    poses = [p.to(dev) for p in synthetic.candidate_poses(V, 2)]
    Z = torch.randn(((F + V) * K, 3, S, S), device=dev, generator=torch.Generator(device=dev).manual_seed(P))
    cursor = [0]

    def hand_out(n, zs=None, _Z=Z, _c=cursor):
        z = _Z[_c[0]:_c[0] + n]
        _c[0] += n
        assert z.shape[0] == n, "more probes drawn than one call of either route takes"
        return z
    slam._draw_probes = hand_out

    def run(fused, crit):
        cursor[0] = 0
        return slam.pose_eval_popgs_blocks(poses, criterion=crit, K=K, lam=args.lam, fused=fused)[0]

    res = {}
    for crit in ("topt", "dopt"):
        run(True, crit); run(False, crit)                          # warm-up of every shape
        t = {True: [], False: []}
        for _ in range(args.reps):
            for fused in (True, False):
                t[fused].append(timed(lambda: run(fused, crit))[0])
        s_new, s_old = run(True, crit).double().numpy(), run(False, crit).double().numpy()
        both = np.isfinite(s_new) & np.isfinite(s_old)
        rel = float(np.max(np.abs(s_new - s_old)[both] / np.abs(s_new)[both])) if both.any() else float("nan")
        n, o = spread(t[True]), spread(t[False])
        kn, hn = counted(lambda: run(True, crit))
        ko, ho = counted(lambda: run(False, crit))
        res[crit] = dict(fused=n, unfused=o, kernels=dict(fused=kn, unfused=ko), device_to_host_copies=dict(fused=hn, unfused=ho),
                         max_rel_difference_of_the_scores=rel, poses_scored_finite=int(both.sum()))
        say(f"P = {P}, {V} poses, K = {K}, {crit}: fused=True {n['median_ms']:.2f} ms [{n['min_ms']:.2f} .. {n['max_ms']:.2f}]"
            f"   fused=False {o['median_ms']:.2f} ms [{o['min_ms']:.2f} .. {o['max_ms']:.2f}]   ratio {o['median_ms'] / n['median_ms']:.2f}"
            f"   separated: {n['max_ms'] < o['min_ms']}")
        say(f"  per call: kernels {kn} against {ko}, device-to-host copies {hn} against {ho};"
            f" scores (float32 out) differ by at most {rel:.2e} relative over {int(both.sum())} poses")
    result[f"P{P}"] = res
    del slam, params, Z
    torch.cuda.empty_cache()

os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "popgs_block_bench.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
print(json.dumps(dict(wrote=os.path.join(args.out_dir, "popgs_block_bench.txt"), result=result)))
