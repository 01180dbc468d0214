#!/usr/bin/env python3
"""tools/target_select_bench.py [out.txt] [--quick]

What the target selection of global_planning costs on the device (fisher_rast.cluster.select_target / dbscan_labels over
fr_target_select / fr_dbscan) beside the chain it replaces (models/SLAM/gaussian.py:1221-1267: torch boolean indexing and
torch.quantile on the device, a copy to the host, sklearn.cluster.DBSCAN(eps=0.1, min_samples=5), the Python loop over the labels),
with sklearn on this machine's host CPU.

The map is fisher_rast.synthetic.room_shell(P) with the whole height of the room as the band, so the points above the 0.8 quantile
are 20 % of P: 20k, 100k and 400k selected points at P = 100k, 500k and 2M.  The scores are a smooth field over the room plus
noise, so that the selected points lie together in regions, as high-uncertainty Gaussians do, rather than being scattered.

  * select_target: a host clock around ITERS calls (each ends in its one host read of the status block);
  * dbscan_labels on the selected points alone: HIP events around ITERS calls;
  * the reference chain: a host clock around one call (the torch part on the device, ending in its copies to the host; sklearn
    on the host), the sklearn part also alone.

Launches per call are counted from the entry points' structure (the sort's count depends on the capacity).  When sklearn is not
installed the tool says so and quotes figures measured elsewhere.  No speed-up is asserted: the ratios are reported."""
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
from fisher_rast import cluster, synthetic                 # noqa: E402

try:
    from sklearn.cluster import DBSCAN
    import sklearn
except ImportError:
    DBSCAN = None

QUICK = "--quick" in sys.argv
REPS, ITERS = (2, 2) if QUICK else (5, 10)
SIZES = (100_000,) if QUICK else (100_000, 500_000, 2_000_000)
LOWER_Y, UPPER_Y, Q, EPS, MIN_SAMPLES = -2.0, 2.0, 0.8, 0.1, 5
ELSEWHERE = {20_000: 0.14, 100_000: 1.28}        # seconds, sklearn 1.7.2 alone on anisotropic blobs, one run on another machine's CPU
dev = torch.device("cuda:0")
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def fmt(v):
    v = sorted(v)
    return f"{v[len(v) // 2]:9.3f} ms [{v[0]:.3f} .. {v[-1]:.3f}]"


def med(v):
    return sorted(v)[len(v) // 2]


def device_ms(step):
    step()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            step()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / ITERS)
    return out


def host_ms(step, iters=None, reps=None):
    iters, reps = iters or ITERS, reps or REPS
    step()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def sort_launches(n):
    """fr_sort_keys64: one chunk sort, then per doubling above 2048 keys one global step per stride down to 2048 and one chunk merge"""
    if n == 0:
        return 0
    n_pad, count, k = 1, 1, 4096
    while n_pad < n:
        n_pad <<= 1
    while k <= n_pad:
        j = k >> 2
        count += 2
        while j >= 2048:
            count += 1
            j >>= 1
        k <<= 1
    return count


def dbscan_launches(cap):
    return 2 + 10 + sort_launches(cap)               # two memsets of the accumulators, ten kernels, the sort


def select_launches(P):
    return 3 + 3 * 3 + 6 + dbscan_launches(P) + 1 + 2   # memsets; three compactions; four histograms, next, threshold; DBSCAN; cmax memset; cmax, winner


def make_map(P):
    means = synthetic.room_shell(P, seed=3)["means3D"]
    g = torch.Generator().manual_seed(17)
    field = torch.sin(0.9 * means[:, 0] + 0.4) * torch.cos(0.7 * means[:, 2] - 0.3) + 0.3 * torch.sin(2.1 * means[:, 1])
    scores = (1.5 + field + 0.15 * torch.randn((P,), generator=g)).float()
    return means.to(dev), scores.to(dev)


def reference_chain(means, scores, timings=None):
    """gaussian.py:1221-1267 without the npz dump: returns (n_above, n_clusters, max_label, n_selected)"""
    sign = torch.bitwise_and(means[:, 1] >= LOWER_Y, means[:, 1] <= UPPER_Y)
    selected_points_xyz = means[sign]
    selected_scores = scores[sign]
    points_index_range = torch.where(sign)[0]
    threshold = torch.quantile(selected_scores, Q)
    above = selected_scores > threshold
    xyz = selected_points_xyz[above]
    points_index = points_index_range[above]
    scores_np = selected_scores[above].cpu().numpy()
    pts_np = xyz.cpu().numpy()
    t0 = time.perf_counter()
    labels = DBSCAN(eps=EPS, min_samples=MIN_SAMPLES).fit(pts_np).labels_
    if timings is not None:
        timings.append((time.perf_counter() - t0) * 1e3)
    max_label, max_score = -1, -1
    for lab in np.unique(labels):
        if lab < 0:
            continue
        cs = scores_np[labels == lab].max()
        if cs > max_score:
            max_label, max_score = lab, cs
    selected_points_index = points_index[torch.from_numpy(labels == max_label).to(points_index.device)]
    return len(pts_np), int(labels.max()) + 1, int(max_label), int(selected_points_index.numel()), labels


def main():
    out_path = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "target_select_bench.txt"))
    say(f"target selection of global_planning: {torch.cuda.get_device_name(0)}, torch {torch.__version__}; "
        f"q = {Q}, eps = {EPS}, min_samples = {MIN_SAMPLES}; median [min .. max] of {REPS} x {ITERS} calls")
    say("sklearn " + (sklearn.__version__ if DBSCAN else "is NOT installed on this machine: the chain is not timed here; measured elsewhere "
                      "(sklearn 1.7.2 alone, anisotropic blobs, one run on a CPU): 0.14 s at 20k points, 1.28 s at 100k"))
    say(f"host CPUs used by this process: {len(os.sched_getaffinity(0))}")
    for P in SIZES:
        means, scores = make_map(P)
        sel = cluster.select_target(means, scores, LOWER_Y, UPPER_Y, Q, EPS, MIN_SAMPLES)
        say()
        say(f"P = {P:,}: band {sel.n_band:,}, above the threshold {sel.n_above:,}, clusters {sel.n_clusters:,}, winner {sel.max_label} "
            f"with {sel.n_selected:,} points; cell sides {tuple(round(s, 4) for s in sel.cell_sides)}")
        t_sel = host_ms(lambda: cluster.select_target(means, scores, LOWER_Y, UPPER_Y, Q, EPS, MIN_SAMPLES))
        pts = means[sel.points_index.long()].contiguous()
        t_db = device_ms(lambda: cluster.dbscan_raw(pts, EPS, MIN_SAMPLES))
        say(f"    select_target (one call, one host read; {select_launches(P)} launches and memsets)   {fmt(t_sel)}")
        say(f"    dbscan_labels on the {sel.n_above:,} selected points ({dbscan_launches(sel.n_above)} launches and memsets)   {fmt(t_db)}")
        if DBSCAN is None:
            near = ELSEWHERE.get(min(ELSEWHERE, key=lambda k: abs(k - sel.n_above)))
            say(f"    torch + sklearn chain: not measured here (sklearn missing); sklearn alone elsewhere at a comparable size: {near * 1e3:.0f} ms")
            continue
        # the chain is timed call by call (the largest size once: sklearn takes a while there); the first call also warms torch up
        alone, t_ref = [], []
        print(f"    (timing the torch + sklearn chain at {sel.n_above:,} points ...)", flush=True)
        for _ in range(1 if P > 500_000 else (2 if QUICK else 3)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            n_above, n_clusters, max_label, n_selected, labels = reference_chain(means, scores, alone)
            torch.cuda.synchronize()
            t_ref.append((time.perf_counter() - t0) * 1e3)
        same = (n_above, n_clusters, max_label, n_selected) == (sel.n_above, sel.n_clusters, sel.max_label, sel.n_selected)
        diff = int((labels != sel.labels.cpu().numpy()).sum()) if n_above == sel.n_above else -1
        say(f"    torch + sklearn.DBSCAN chain, {len(t_ref)} call(s) (a host synchronisation per boolean indexing and copy)   {fmt(t_ref)}   "
            f"of which sklearn alone {fmt(alone)}")
        say(f"    ratio chain / select_target: {med(t_ref) / med(t_sel):.1f} x;   sklearn alone / dbscan_labels: {med(alone) / med(t_db):.1f} x")
        say(f"    same counts and winner as the chain: {same};  labels that differ from sklearn's: {diff} of {n_above:,} "
            "(binary32 distances: a pair within rounding of eps may fall on the other side)")
    with open(out_path, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_path}")


if __name__ == "__main__":
    main()
