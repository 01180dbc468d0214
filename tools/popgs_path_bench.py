#!/usr/bin/env python3
"""POp-GS path evaluation (tester_gaussians_navigation.py:2109-2204) at the benchmark size: BASELINE.json configs[1]'s map with 11
Fisher columns (room_shell 500k, seed 2, 256 x 256), 21 paths x 30 actions, acc_H_train_every = 5, K = 4.

One process, every shape warmed up first, the two sides of a comparison alternating, host clock around a synchronise:
  (a) the criterion step of ONE round on probe rows that are already there: fr_popgs_diag_criterion against the torch chain it
      replaces (`_flat_diag` -> `_diag_scores` -> `H_path + cur`), for both criteria, for the first round (one shared prior) and for
      a later one (a prior per path, updated in place);
  (b) the whole `evaluate_paths_popgs` against the serial loop over `estimate_diag_JtJ_simple` at every step.
Beside them the device copy rate as bench.py measures it and the kernel's algorithmic bytes 4 E (V K + V_prior + V_written).
Writes <out-dir>/popgs_path_bench.{txt,json}.  `--criterion-only` leaves (b) out: the form to run under
`rocprofv3 --kernel-trace --stats -- python3 tools/popgs_path_bench.py --criterion-only` for the kernel's own time."""
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
ap.add_argument("--P", type=int, default=500_000)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--paths", type=int, default=21)
ap.add_argument("--actions", type=int, default=30)
ap.add_argument("--acc", type=int, default=5)
ap.add_argument("--K", type=int, default=4)
ap.add_argument("--lam", type=float, default=1e-6)
ap.add_argument("--reps", type=int, default=7, help="alternating repeats of the criterion step")
ap.add_argument("--path-reps", type=int, default=2, help="alternating repeats of the whole evaluation")
ap.add_argument("--criterion-only", action="store_true")
ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
args = ap.parse_args()

entry.build()
from bench import measured_copy_bandwidth   # noqa: E402
from fisher_rast import ops, synthetic      # noqa: E402
from fisher_rast.path_eval import compute_next_campos, evaluate_paths_popgs, popgs_rows_from_flat   # noqa: E402
import models.gaussian_slam as mgs          # noqa: E402

dev = torch.device("cuda:0")
P, S, V, K, lam = args.P, args.size, args.paths, args.K, args.lam
E = 11 * P
lines = []


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


params = {k: v.to(dev) for k, v in synthetic.room_shell(P, 2).items()}
slam = mgs.GaussianObjectSLAM(params=params, intrinsics=synthetic.intrinsics(S, S), width=S, height=S, device=dev)
for kf in synthetic.invert_rigid(synthetic.candidate_poses(4, 102)):
    slam.add_keyframe(kf.to(dev))
torch.manual_seed(0)
H_train = slam.compute_H_train_popgs(K=K)                       # flat, the reference's block order
prior_rows = popgs_rows_from_flat(H_train, P).reshape(-1)       # the same numbers in the row layout
result = dict(config=dict(P=P, image=[S, S], paths=V, actions=args.actions, acc_H_train_every=args.acc, K=K, lam=lam, E=E,
                          map="room_shell seed 2, 11 Fisher columns (BASELINE.json configs[1]'s map)"))

copy_gbs = measured_copy_bandwidth(dev)
result["copy_rate_GBs"] = copy_gbs
say(f"device copy rate (read + write, bench.measured_copy_bandwidth): {copy_gbs:.0f} GB/s")

# ---- (a) the criterion step of one round ------------------------------------------------------------------------------
w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, 2)).to(dev)
rows, vis = slam._pose_probe_rows(w2c, K)                       # [V, K, P, 11]
vis = vis.to(torch.int32).contiguous()
ones = torch.ones((V,), dtype=torch.uint8, device=dev)
state = torch.empty((V, E), dtype=torch.float32, device=dev)
ws = torch.empty((V * 96,), dtype=torch.float64, device=dev)
scores = torch.empty((V,), dtype=torch.float64, device=dev)
say(f"one round: {V} paths x K = {K} probes x E = {E} entries: rows {rows.numel() * 4 / 1e9:.2f} GB, state {state.numel() * 4 / 1e9:.2f} GB")


def new_first(crit):            # round 0: one shared prior in, a prior per path out
    return ops.popgs_diag_criterion(rows, prior_rows, lam, crit, prior_out=state, accumulate=ones, vis_count=vis, scores=scores, workspace=ws)


def new_later(crit):            # round m > 0: a prior per path, updated in place
    return ops.popgs_diag_criterion(rows, state, lam, crit, prior_out=state, accumulate=ones, vis_count=vis, scores=scores, workspace=ws)


def torch_first(crit):          # the chain at the parent commit: batched criteria against the shared prior, then H_path + cur
    diags = slam._flat_diag(rows)
    s = slam._diag_scores(H_train, diags, lam, crit)
    return s, H_train.unsqueeze(0) + diags


H_paths = None


def torch_later(crit):          # a prior per path: `_diag_scores` takes one prior, so path by path as evaluate_paths does
    global H_paths
    diags = slam._flat_diag(rows)
    s = torch.stack([slam._diag_scores(H_paths[v], diags[v:v + 1], lam, crit)[0] for v in range(V)])
    H_paths = [H_paths[v] + diags[v] for v in range(V)]
    return s


crit_res = {}
for crit in ("topt", "dopt"):
    H_paths = [H_train.clone() for _ in range(V)]
    new_first(crit); torch_first(crit); new_later(crit); torch_later(crit)          # warm-up of every shape
    t = {k: [] for k in ("new_first", "torch_first", "new_later", "torch_later")}
    for _ in range(args.reps):
        t["new_first"].append(timed(lambda: new_first(crit))[0])
        t["torch_first"].append(timed(lambda: torch_first(crit))[0])
        t["new_later"].append(timed(lambda: new_later(crit))[0])
        t["torch_later"].append(timed(lambda: torch_later(crit))[0])
    # the two routes on the same rows and prior: how far apart the scores are
    s_new = new_first(crit).cpu().numpy()
    s_old = torch_first(crit)[0].double().cpu().numpy()
    s_old = np.where(vis.cpu().numpy() == 0, 0.0, s_old)
    dev_rel = float(np.max(np.abs(s_new - s_old) / np.maximum(np.abs(s_old), 1e-300)))
    crit_res[crit] = {k: spread(v) for k, v in t.items()}
    crit_res[crit]["max_rel_difference_new_vs_torch_fp32"] = dev_rel
    for form in ("first", "later"):
        n, o = crit_res[crit]["new_" + form], crit_res[crit]["torch_" + form]
        say(f"criterion step, {crit}, {form} round: fr_popgs_diag_criterion {n['median_ms']:.3f} ms [{n['min_ms']:.3f} .. {n['max_ms']:.3f}]"
            f"   torch chain {o['median_ms']:.3f} ms [{o['min_ms']:.3f} .. {o['max_ms']:.3f}]   ratio {o['median_ms'] / n['median_ms']:.2f}"
            f"   separated: {n['max_ms'] < o['min_ms']}")
    say(f"  scores, new (fp32 terms, fp64 sums) against the torch chain (fp32 sums): max relative difference {dev_rel:.2e}")
    del H_paths
    H_paths = None
result["criterion_step"] = crit_res
alg = {"first": 4 * E * (V * K + 1 + V), "later": 4 * E * (V * K + V + V)}
result["algorithmic_bytes"] = alg
for form in ("first", "later"):
    for crit in ("topt", "dopt"):
        ms = crit_res[crit]["new_" + form]["median_ms"]
        say(f"algorithmic bytes, {form} round: {alg[form] / 1e9:.3f} GB; {crit} call (both kernels, host clock) {ms:.3f} ms -> "
            f"{alg[form] / ms / 1e6:.0f} GB/s = {alg[form] / ms / 1e6 / copy_gbs:.2f} of the copy rate")
del rows, state
torch.cuda.empty_cache()

# ---- (b) the whole evaluation -----------------------------------------------------------------------------------------
if not args.criterion_only:
    rng = np.random.default_rng(5)
    start = synthetic.candidate_poses(1, 3)[0].numpy().astype(np.float64)
    paths = [list(rng.integers(1, 4, size=args.actions)) for _ in range(V)]
    finals = [0.0] * V

    def serial(paths, crit):
        """tester 2121-2191 on this repository's estimator: one estimate_diag_JtJ_simple per step, the criterion as torch ops."""
        out = []
        for actions in paths:
            H_path = H_train.clone()
            pose, total, done = start.copy(), 0.0, 0
            for a in actions:
                pose = compute_next_campos(pose, int(a))
                cur, vis_count = slam.estimate_diag_JtJ_simple(np.linalg.inv(pose), K)
                Hm = H_path + lam
                Hpi = Hm + cur
                if vis_count == 0:
                    e = torch.tensor(0.)
                elif crit == "topt":
                    e = -torch.sum(1.0 / torch.clamp(Hpi, min=1e-12))
                else:
                    e = torch.sum(torch.log(torch.clamp(Hpi, min=1e-12))) - torch.sum(torch.log(torch.clamp(Hm, min=1e-12)))
                done += 1
                if (done + 1) % args.acc == 0:
                    total += float(e.item())
                    H_path = H_path + cur
            out.append((total + 0.0) / max(done, 1))
        return out

    def batched(paths, crit):
        return evaluate_paths_popgs(slam, start, paths, [0.0] * len(paths), H_train, criterion=crit, lam=lam, K=K,
                                    acc_H_train_every=args.acc)

    crit = "topt"
    batched(paths, crit)                                             # warm-up at the full shape (workspaces grow to it)
    serial([p[:args.acc] for p in paths[:2]], crit)                  # warm-up: the serial loop has one shape
    tb, tsr = [], []
    for _ in range(args.path_reps):
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        tb.append(timed(lambda: batched(paths, crit))[0])
        peak = torch.cuda.max_memory_allocated(dev) - base
        tsr.append(timed(lambda: serial(paths, crit))[0])
    result["whole_evaluation"] = dict(criterion=crit, batched=spread(tb), serial=spread(tsr), peak_bytes_above_map_and_workspaces=peak,
                                      estimator_calls_serial=V * args.actions, probe_launches_batched=args.actions // args.acc)
    say(f"whole evaluation, {V} paths x {args.actions} actions, {crit}: evaluate_paths_popgs {statistics.median(tb):.1f} ms {[round(x, 1) for x in tb]}"
        f"   serial loop {statistics.median(tsr):.1f} ms {[round(x, 1) for x in tsr]}   ratio {statistics.median(tsr) / statistics.median(tb):.2f}")
    say(f"  peak device memory of the batched call above what was held before it: {peak / 1e9:.2f} GB (rows {V * K * E * 4 / 1e9:.2f} GB + state {V * E * 4 / 1e9:.2f} GB + probes)")

os.makedirs(args.out_dir, exist_ok=True)
with open(os.path.join(args.out_dir, "popgs_path_bench.txt"), "w") as f:
    f.write("\n".join(lines) + "\n")
with open(os.path.join(args.out_dir, "popgs_path_bench.json"), "w") as f:
    json.dump(result, f, indent=1)
print(json.dumps(dict(wrote=os.path.join(args.out_dir, "popgs_path_bench.json"))))
