#!/usr/bin/env python3
"""tools/recon_stream_bench.py [out.txt] [--quick]

What a navigation step's object evaluation costs when the metrics are carried forward (fisher_rast.cloud.ReconTracker) against
re-evaluating the accumulated cloud (reconstruction_metrics, the route the package had before), as the run gets longer.

Setting: the ground truth is a 200k-point surface cloud (a sphere of radius 0.5 m); every frame is a 256 x 256 depth image of it from
a camera 1.7 m away in a random direction, +-3 mm of depth noise, with the object's mask over about a tenth of the pixels.

  (a) one step of the tracker, add_frame + metrics() (three library calls, one statistics pass, one host read), timed by a host
      clock around each step (metrics() ends in the host read) for the 10 steps that follow 10, 100 and 500 folded frames, in
      RUNS identical runs of 510 frames;
  (b) reconstruction_metrics(gt_index, accumulated cloud) on the cloud the tracker kept after 10, 100 and 500 frames;
  (c) the fold of the ground truth against ONE frame's index, device time: with the seeds 100 earlier frames left, and with
      every seed +inf.

Timing helpers: tools/cloud_nn_bench.py's (HIP events around ITERS calls after a warm-up, or a host clock around calls that end in
a host read; median [min .. max] of REPS repeats)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np   # noqa: E402
import torch         # noqa: E402
import cloud_nn_bench as nb   # noqa: E402  (builds the library, puts the package on the path)
from cloud_nn_bench import say, fmt, med, device_ms, host_ms, dev, QUICK   # noqa: E402
from fisher_rast import cloud   # noqa: E402

N_GT = 20_000 if QUICK else 200_000
S = 64 if QUICK else 256
POINTS = (2, 5, 8) if QUICK else (10, 100, 500)
WINDOW = 2 if QUICK else 10
RUNS = 2 if QUICK else 3
TH = 0.01                             # the reference's threshold for the object (tester_gaussians_navigation.py:1213)
RADIUS, DIST = 0.5, 1.7


def look_at(eye):
    z = -eye / np.linalg.norm(eye)
    x = np.cross(np.array([0.0, 1.0, 0.0]), z)
    x /= np.linalg.norm(x)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = x, np.cross(z, x), z, eye
    return c2w


def make_frames(n, seed=11):
    """[(depth [S,S] float32, mask [S,S] uint8, kinv [3,3], cam_to_eval [4,4])] on the device, made there from a seed"""
    rng = np.random.default_rng(seed)
    gen = torch.Generator(device=dev).manual_seed(seed)
    fx = 0.6 * S
    K = np.array([[fx, 0, S / 2 - 0.5], [0, fx, S / 2 - 0.5], [0, 0, 1]])
    kinv = torch.from_numpy(np.linalg.inv(K)).float().to(dev)
    v, u = torch.meshgrid(torch.arange(S, device=dev, dtype=torch.float64), torch.arange(S, device=dev, dtype=torch.float64), indexing="ij")
    rays = torch.stack([(u - K[0, 2]) / fx, (v - K[1, 2]) / fx, torch.ones_like(u)], -1)
    frames = []
    for _ in range(n):
        d = rng.normal(size=3)
        d[1] *= 0.5
        c2w = look_at(DIST * d / np.linalg.norm(d))
        R, o = torch.from_numpy(c2w[:3, :3]).to(dev), torch.from_numpy(c2w[:3, 3]).to(dev)
        rw = rays @ R.T
        a, b, c = (rw * rw).sum(-1), 2 * (rw @ o), float(o @ o) - RADIUS ** 2
        disc = b * b - 4 * a * c
        hit = disc > 0
        depth = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / (2 * a), torch.full_like(a, 3.0))
        depth = depth + (torch.rand((S, S), device=dev, generator=gen, dtype=torch.float64) - 0.5) * 0.006
        frames.append((depth.float().contiguous(), hit.to(torch.uint8).contiguous(), kinv, torch.from_numpy(c2w).float().to(dev)))
    torch.cuda.synchronize()
    return frames


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "recon_stream_bench.txt"))
    say(f"recon_stream_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, REPS {nb.REPS} ITERS {nb.ITERS} RUNS {RUNS}"
        f"{' (quick)' if QUICK else ''}")
    rng = np.random.default_rng(3)
    g = rng.normal(size=(N_GT, 3))
    gt = cloud.CloudIndex(torch.from_numpy((RADIUS * g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)).to(dev))
    n_frames = POINTS[-1] + WINDOW
    frames = make_frames(n_frames)
    share = float(np.mean([float(f[1].float().mean()) for f in frames[:20]]))
    say(f"ground truth {N_GT:,} points; {n_frames} frames of {S} x {S}, mask over {100 * share:.1f} % of the pixels; dist_th {TH}")

    # (a) the tracker, step by step
    tracker = cloud.ReconTracker(gt, TH, keep_points=True)
    clouds, seeds, per_run, m_at = {}, {}, [], {}
    for run in range(RUNS + 1):                                  # run 0 warms up and keeps the clouds for (b) and the seeds for (c)
        tracker.reset()
        step_ms = []
        for i, (depth, mask, kinv, T) in enumerate(frames):
            if run == 0 and i in POINTS:
                clouds[i] = tracker.cloud().clone()
                seeds[i] = tracker.best_d2.clone()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tracker.add_frame(depth, kinv, T, mask=mask)
            m = tracker.metrics()
            step_ms.append((time.perf_counter() - t0) * 1e3)
            if run == 0 and i + 1 in POINTS:
                m_at[i + 1] = m
        if run:
            per_run.append(step_ms)
    say()
    say(f"(a) ReconTracker: add_frame + metrics(), host clock per step, the {WINDOW} steps after n folded frames, {RUNS} identical runs")
    a_med = {}
    for n in POINTS:
        per = [sorted(r[n:n + WINDOW])[WINDOW // 2] for r in per_run]
        allv = [v for r in per_run for v in r[n:n + WINDOW]]
        a_med[n] = med(per)
        say(f"    after {n:>3} frames: {fmt(allv)}   medians of the runs: {', '.join(f'{v:.3f}' for v in per)}")
    spread = max(max(sorted(r[n:n + WINDOW])[WINDOW // 2] for r in per_run) - min(sorted(r[n:n + WINDOW])[WINDOW // 2] for r in per_run) for n in POINTS)
    say(f"    largest spread of a point's median across identical runs {spread:.3f} ms; medians across the points differ by "
        f"{max(a_med.values()) - min(a_med.values()):.3f} ms")

    # (b) today's route on the accumulated cloud
    say()
    say("(b) reconstruction_metrics(gt_index, accumulated cloud): one build, two searches, two reductions, one host read")
    b_med = {}
    for n in POINTS:
        rec = clouds[n]
        t = host_ms(lambda: cloud.reconstruction_metrics(gt, rec, TH), iters=max(2, nb.ITERS // 2))
        b_med[n] = med(t)
        want, got = cloud.reconstruction_metrics(gt, rec, TH), m_at[n]
        same = all(got[k] == want[k] for k in ("comp", "ratio", "iratio", "fpr")) and abs(got["acc"] - want["acc"]) <= 2 * got["n_rec"] * 2.0 ** -53 * want["acc"]
        say(f"    after {n:>3} frames ({rec.shape[0]:>9,} points): {fmt(t)}   the tracker's numbers at that point are these: {same}")
        say(f"        acc {want['acc']:.6f} comp {want['comp']:.6f} ratio {want['ratio']:.6f} iratio {want['iratio']:.6f}")
    say(f"    (b) grows {b_med[POINTS[-1]] / b_med[POINTS[0]]:.1f}x from {POINTS[0]} to {POINTS[-1]} frames; (a) {a_med[POINTS[-1]] / a_med[POINTS[0]]:.2f}x")

    # (c) the fold alone
    say()
    n = POINTS[1]
    depth, mask, kinv, T = frames[n]
    pts = gt.query_depth(depth, kinv, T, dist_th=TH, mask=mask, near=True, want_points=True)[2]
    fix = cloud.CloudIndex(pts)
    work = torch.empty_like(seeds[n])
    inf = torch.full_like(work, float("inf"))
    say(f"(c) fold of the {N_GT:,} ground-truth points against one frame's index ({int(torch.isfinite(pts).all(1).sum()):,} finite of {pts.shape[0]:,} rows), "
        f"device time, the seeds restored before every fold (the copy is inside both figures)")
    copy = device_ms(lambda: work.copy_(inf))
    res = {}
    for _ in range(2):                                          # alternating, as two versions measured in one call
        for name, src in ((f"seeds left by {n} earlier frames", seeds[n]), ("every seed +inf", inf)):
            res.setdefault(name, []).extend(device_ms(lambda: (work.copy_(src), fix.fold(gt.points, work))))
    for name, v in res.items():
        say(f"    {name:<34} {fmt(v)}")
    say(f"    {'the copy alone':<34} {fmt(copy)}")
    work.copy_(seeds[n])
    fix.fold(gt.points, work)
    improved = int((work < seeds[n]).sum())
    say(f"    ground-truth points this frame improved with the finite seeds: {improved:,} of {N_GT:,}")
    a_name, b_name = list(res)
    say(f"    finite seeds not slower than +inf beyond the spread: {med(res[a_name]) <= med(res[b_name]) + (max(res[b_name]) - min(res[b_name]))}")

    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(nb.LINES) + "\n")


if __name__ == "__main__":
    main()
