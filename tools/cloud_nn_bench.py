#!/usr/bin/env python3
"""tools/cloud_nn_bench.py [out.txt] [--quick]

What the nearest-point search (fr_cloud_index_build / fr_cloud_query under fisher_rast/cloud.py) costs against the route the
reference takes on the host, SciPy KD-trees rebuilt on every call, on the same machine's CPU:

  (a) the index build at 500k, 1M and 2M targets;
  (b) reconstruction_metrics at 500k x 500k and 2M x 2M: synthetic.room_shell means against the same means jittered by N(0, 2 cm)
      with 10 % strays -- the whole call (two builds, two searches, two reductions, one host read), and build / search / reduction
      separately.  Reference route: accuracy_comp_ratio_from_pcl builds three KD-trees and runs three queries, and the tester
      calls it twice with swapped arguments; ONE call is timed and doubled, as the reference calls it (workers=1) and with workers=16;
  (c) novelty_mask_from_pcd_nn at 256^2 and 512^2, stride 1, against a 1M-point room cloud, with a prebuilt CloudIndex and with
      the index built in the call.  Reference route: cKDTree over the cloud + query (the reference asks for workers=-1; also 16).

Device times are HIP events around ITERS calls after a warm-up, median [min .. max] of REPS repeats; calls that end in a host read
are timed by a host clock around ITERS calls (each call synchronises).  "reduction" is (search + statistics) - (search alone).
The share of the search spent on the linear scan of the top-level boxes at 2M is bounded from above: queries that COINCIDE with
targets reject every box at the top level but the few that contain them, so (that search - the query sort) / (the search - the
query sort) bounds it, with the query sort measured as a search against a 64-point index.

Required, and asserted: every GPU time is below the workers=16 SciPy time of the same case."""
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
from fisher_rast import cloud, synthetic                   # noqa: E402
from scipy.spatial import KDTree, cKDTree                  # noqa: E402

QUICK = "--quick" in sys.argv
REPS, ITERS = (2, 2) if QUICK else (5, 10)
TH = 0.05
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


def device_ms(step, iters=None):
    """HIP events around `iters` calls, per call; REPS repeats after a warm-up"""
    iters = iters or ITERS
    step()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            step()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return out


def host_ms(step, iters=None):
    iters = iters or ITERS
    step()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        for _ in range(iters):
            step()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / iters)
    return out


def clouds(n, seed=3):
    gt = synthetic.room_shell(n, seed=seed)["means3D"].numpy()
    rng = np.random.default_rng(seed)
    rec = gt + rng.normal(0, 0.02, gt.shape).astype(np.float32)
    stray = rng.uniform(size=n) < 0.10
    rec[stray] = rng.uniform(-1, 1, (int(stray.sum()), 3)).astype(np.float32) * np.array([5.5, 1.5, 5.5], np.float32)
    return gt, rec.astype(np.float32)


def scipy_metrics_call(gt, rec, th, workers):
    """the three trees and three queries of ONE accuracy_comp_ratio_from_pcl; seconds for build and for query"""
    tb = tq = 0.0
    vals = []
    for a, b in ((gt, rec), (rec, gt), (rec, gt)):          # accuracy: tree over gt; completion and ratio: tree over rec
        t0 = time.perf_counter()
        tree = KDTree(a)
        t1 = time.perf_counter()
        d, _ = tree.query(b, workers=workers)
        t2 = time.perf_counter()
        tb, tq = tb + (t1 - t0), tq + (t2 - t1)
        vals.append(d)
    return tb, tq, (float(np.mean(vals[0])), float(np.mean(vals[1])), float(np.mean((vals[2] < th).astype(float))))


def part_a():
    say("(a) index build (fr_cloud_index_build), device time")
    for n in ((100_000,) if QUICK else (500_000, 1_000_000, 2_000_000)):
        pts = synthetic.room_shell(n, seed=3)["means3D"].to(dev)
        say(f"    N = {n:>9,}: {fmt(device_ms(lambda: cloud.CloudIndex(pts)))}")


def part_b():
    say()
    say("(b) reconstruction_metrics(gt, rec, 0.05): room_shell means against themselves + N(0, 2 cm), 10 % strays")
    worst_ok = True
    for n in ((100_000,) if QUICK else (500_000, 2_000_000)):
        gt, rec = clouds(n)
        gtd, recd = torch.from_numpy(gt).to(dev), torch.from_numpy(rec).to(dev)
        whole = host_ms(lambda: cloud.reconstruction_metrics(gtd, recd, TH), iters=max(2, ITERS // 2))
        got = cloud.reconstruction_metrics(gtd, recd, TH)
        build = device_ms(lambda: cloud.CloudIndex(gtd))
        gix, rix = cloud.CloudIndex(gtd), cloud.CloudIndex(recd)
        search = device_ms(lambda: gix.search(recd, TH))
        search_stats = device_ms(lambda: gix.search(recd, TH, dist=False, stats=True))
        say(f"    {n:,} x {n:,}")
        say(f"      whole call (2 builds + 2 searches + 2 reductions + host read)   {fmt(whole)}")
        say(f"      one build                                                      {fmt(build)}")
        say(f"      one search (query keys + sort + search, distances written)     {fmt(search)}")
        say(f"      one search + statistics                                        {fmt(search_stats)}")
        say(f"      reduction = the difference                                     {med(search_stats) - med(search):9.3f} ms")
        if n >= 2_000_000 or QUICK:
            tiny = cloud.CloudIndex(gtd[:64].contiguous())
            sort_only = device_ms(lambda: tiny.search(recd, TH))
            exact = device_ms(lambda: gix.search(gtd, TH))
            share = (med(exact) - med(sort_only)) / max(med(search) - med(sort_only), 1e-9)
            say(f"      query keys + sort alone (search against a 64-point index)     {fmt(sort_only)}")
            say(f"      search of queries that coincide with targets                  {fmt(exact)}")
            say(f"      top-level linear scan: at most {100 * share:.0f} % of the search proper ({med(exact) - med(sort_only):.3f} of {med(search) - med(sort_only):.3f} ms)")
        for workers in (1, 16):
            tb, tq, want = scipy_metrics_call(gt, rec, TH, workers)
            say(f"      SciPy KDTree, workers={workers:<2}: one call {1e3 * (tb + tq):10.1f} ms (3 builds {1e3 * tb:.1f} + 3 queries {1e3 * tq:.1f}); "
                f"the tester's two calls {2e3 * (tb + tq):10.1f} ms")
            if workers == 16:
                ok = max(whole) < 2e3 * (tb + tq)
                worst_ok &= ok
                say(f"      GPU whole call below the workers=16 route: {ok}  ({2e3 * (tb + tq) / med(whole):.0f}x)")
        rel = max(abs(got["acc"] - want[0]) / want[0], abs(got["comp"] - want[1]) / want[1])
        say(f"      acc {got['acc']:.6f} comp {got['comp']:.6f} ratio {got['ratio']:.6f} iratio {got['iratio']:.6f}; against SciPy: acc / comp rel {rel:.1e}, "
            f"ratio {'equal' if got['ratio'] == want[2] else 'DIFFERS ' + repr(want[2])}")
    return worst_ok


def room_depth(S, c2w):
    """the depth image (z along the optical axis, +Z forward) of the empty room x,z in [-5,5], y in [-1.25,1.25] from c2w, and inv_K"""
    fx = 0.6 * S
    K = np.array([[fx, 0, S / 2 - 0.5], [0, fx, S / 2 - 0.5], [0, 0, 1]])
    v, u = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    rays = np.stack([(u - K[0, 2]) / fx, (v - K[1, 2]) / fx, np.ones_like(u, float)], -1) @ c2w[:3, :3].T
    o, half = c2w[:3, 3], np.array([5.0, 1.25, 5.0])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(rays > 0, (half - o) / rays, (-half - o) / rays)
    depth = np.nanmin(np.where(np.isfinite(t) & (t > 0), t, np.inf), -1)
    depth[S // 3:S // 2, S // 3:S // 2] *= 0.6                 # something the environment cloud does not hold
    depth[:4] = 0.0                                            # unmeasured rows
    inv_K = np.eye(4)
    inv_K[:3, :3] = np.linalg.inv(K)
    return depth.astype(np.float32), inv_K.astype(np.float32)


def part_c():
    say()
    say("(c) novelty_mask_from_pcd_nn, stride 1, 5 cm, against a room cloud")
    n = 100_000 if QUICK else 1_000_000
    env = synthetic.room_shell(n, seed=5)["means3D"]
    env = env[(env.abs() / torch.tensor([5.0, 1.25, 5.0])).max(1).values > 0.98].contiguous()      # the faces: the surface a depth camera sees
    envd = env.to(dev)
    yaw = 0.4
    c2w = np.eye(4)
    c2w[:3, :3] = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    c2w[:3, 3] = [0.5, 0.1, -1.0]
    c2w_t = torch.from_numpy(c2w.astype(np.float32))
    ix = cloud.CloudIndex(envd)
    ok_all = True
    say(f"    environment cloud: {env.shape[0]:,} points")
    for S in (256, 512):
        depth, inv_K = room_depth(S, c2w)
        inv_K_t = torch.from_numpy(inv_K)
        args = (depth, inv_K_t, c2w_t, (S, S), "Z", TH, 1)
        pre = host_ms(lambda: cloud.novelty_mask_from_pcd_nn(ix, *args))
        fresh = host_ms(lambda: cloud.novelty_mask_from_pcd_nn(envd, *args))
        kernel = device_ms(lambda: ix.query_depth(torch.from_numpy(depth).to(dev), cloud.novelty_kinv(inv_K_t), c2w_t, 1, False, TH))
        mask = cloud.novelty_mask_from_pcd_nn(ix, *args)
        say(f"    {S} x {S}: prebuilt index {fmt(pre)}   index built in the call {fmt(fresh)}")
        say(f"             (upload + search + reduction without the host read: {fmt(kernel)}); novel pixels {int(mask.sum()):,}")
        # the reference route: its own arithmetic up to the points, then the tree
        d = torch.from_numpy(depth)
        valid = torch.isfinite(d) & (d > 0)
        vv, uu = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
        kinv = cloud.novelty_kinv(inv_K_t)
        pc = (kinv @ torch.stack([uu[valid].float(), vv[valid].float(), torch.ones(int(valid.sum()))])).t() * d[valid].unsqueeze(1)
        pw = (c2w_t @ torch.cat([pc, torch.ones((pc.shape[0], 1))], 1).t()).t()[:, :3].numpy()
        P_env = env.numpy()
        for workers in (-1, 16):
            t0 = time.perf_counter()
            tree = cKDTree(P_env)
            t1 = time.perf_counter()
            dists, _ = tree.query(pw, k=1, workers=workers)
            t2 = time.perf_counter()
            say(f"             SciPy cKDTree, workers={workers:<2}: {1e3 * (t2 - t0):9.1f} ms (build {1e3 * (t1 - t0):.1f} + query {1e3 * (t2 - t1):.1f})")
            if workers == 16:
                ok = max(pre) < 1e3 * (t2 - t0) and max(fresh) < 1e3 * (t2 - t0)
                ok_all &= ok
                say(f"             both GPU routes below the workers=16 route: {ok}  ({1e3 * (t2 - t0) / med(pre):.0f}x prebuilt, {1e3 * (t2 - t0) / med(fresh):.0f}x built in the call)")
        want = np.zeros((S, S), np.uint8)
        want[valid.numpy()] = dists > TH
        near = int((np.abs(dists - TH) < 1e-4).sum())
        say(f"             mask against the SciPy route: {int((want != mask).sum())} of {S * S} pixels differ ({near} distances within 1e-4 m of the threshold)")
    return ok_all


def main():
    out = next((a for a in sys.argv[1:] if not a.startswith("--")), os.path.join(ROOT, "profiles", "cloud_nn_bench.txt"))
    say(f"cloud_nn_bench: {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {os.cpu_count()} host CPUs visible, "
        f"REPS {REPS} ITERS {ITERS}{' (quick)' if QUICK else ''}")
    part_a()
    ok_b = part_b()
    ok_c = part_c()
    say()
    say(f"every GPU time below the workers=16 SciPy time of the same case: {ok_b and ok_c}")
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    assert ok_b and ok_c, "a GPU time was not below the workers=16 SciPy time"


if __name__ == "__main__":
    main()
