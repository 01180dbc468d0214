#!/usr/bin/env python3
"""tools/map_edit_bench.py [out.json] [--sizes 20000,2000000] [--no-trace] | --kernels-only fused|torch --op prune|densify --iters K [--size P]

What the map edit (fr_map_edit_plan / fr_map_edit_apply / fr_map_edit_split_children) costs against the torch chain it replaces:
one `prune_gaussians` and one `densify` (num_to_split_into = 2) of the mapping loop on an anisotropic map of 20k and of 2M
Gaussians with Adam state on every parameter; about 10 % of the rows are removed by opacity, 5 % cloned, 5 % split.
  fused   models/SLAM/utils/slam_external.prune_gaussians / densify of this package
  torch   the chain the reference runs (models/SLAM/utils/slam_external.py:203-262, 345-463), written out below in this tool's own
          form and in the reference's order: boolean indexing of every parameter, of both Adam moments of each and of the
          statistics per remove_points; per densify two rounds of cats, build_rotation, bmm, three remove_points-sized passes.
Both routes start every call from the same map, optimizer state and statistics (`seen` is all false, so the accumulation both
routes begin densify with adds nothing).  Per route: ITERS calls between two device events (event ms / call) and inside a host
clock that ends in a device synchronise (wall ms / call); REPS alternating repeats after a warm-up; median [min .. max].  Host
synchronisations per call are what torch's sync debug mode reports during one call.

Launch counts come from kernel traces in child processes of their own, after the timing (tracing slows the host): per route and
operation the tool runs
  rocprofv3 --kernel-trace --output-format csv -d <dir> -- python3 tools/map_edit_bench.py --kernels-only <route> --op <op> --iters 10
and the same with --iters 20; (kernels in the second trace - kernels in the first) / 10 = launches per call.  The kernels of this
library among them are counted by name: the map-edit kernels (k_edit_*) and the mask / statistics kernels in front of them
(k_prune_mask, k_densify_*).  --no-trace leaves that part out."""
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
from models.SLAM.utils import slam_external as se    # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS = 7
MAP_KEYS = ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
PRUNE = dict(start_after=0, remove_big_after=100000, stop_after=100000, prune_every=1, removal_opacity_threshold=0.005,
             final_removal_opacity_threshold=0.005, reset_opacities=False, reset_opacities_every=500)
DENSIFY = dict(start_after=0, remove_big_after=100000, stop_after=100000, densify_every=1, grad_thresh=0.0002, num_to_split_into=2,
               removal_opacity_threshold=0.005, final_removal_opacity_threshold=0.005, reset_opacities=False, reset_opacities_every=3000)


class Map:
    """a map of P Gaussians with Adam state, and the means to put it back after a call"""

    def __init__(self, P, seed=7):
        rng = np.random.default_rng(seed)
        u = rng.uniform(size=P)
        lo = rng.normal(3.0, 1.0, (P, 1))
        lo[u < 0.10] = -7.0                                                  # sigmoid < 0.005: removed
        ls = np.log(rng.uniform(0.005, 0.04, (P, 3)))
        v = rng.uniform(size=P)
        ls[v < 0.05, 0] = np.log(rng.uniform(0.06, 0.09, int((v < 0.05).sum())))    # max scale > 0.05: split
        acc = rng.uniform(0, 1e-4, P)
        acc[(v >= 0.05) & (v < 0.10)] = 1e-3                                # gradient over the threshold on a small Gaussian: cloned
        rot = rng.normal(size=(P, 4))
        raw = dict(means3D=rng.uniform(-3, 3, (P, 3)), rgb_colors=rng.uniform(0, 1, (P, 3)), unnorm_rotations=rot, logit_opacities=lo, log_scales=ls,
                   cam_unnorm_rots=np.tile(np.array([1.0, 0, 0, 0])[None, :, None], (1, 1, 2)), cam_trans=np.zeros((1, 3, 2)))
        self.P = P
        self.params = {k: torch.nn.Parameter(torch.tensor(a, dtype=torch.float32, device=dev).contiguous().requires_grad_(True)) for k, a in raw.items()}
        self.optimizer = torch.optim.Adam([dict(params=[p], name=k, lr=1e-3) for k, p in self.params.items()])
        for p in self.params.values():
            p.grad = torch.full_like(p, 1e-3)
        self.optimizer.step()
        for p in self.params.values():
            p.grad = None
        self.saved = {k: (p, dict(self.optimizer.state[p])) for k, p in self.params.items()}
        means2D = torch.zeros((P, 3), device=dev, requires_grad=True)
        means2D.grad = torch.zeros((P, 3), device=dev)
        self.variables = dict(means2D_gradient_accum=torch.tensor(acc, dtype=torch.float32, device=dev), denom=torch.ones(P, device=dev),
                              max_2D_radius=torch.zeros(P, device=dev), timestep=torch.zeros(P, device=dev),
                              seen=torch.zeros(P, dtype=torch.bool, device=dev), means2D=means2D, scene_radius=torch.tensor(3.0, device=dev))

    def fresh(self):
        """(params, variables, optimizer) as they were: the same tensors, the optimizer's groups and state pointed back at them"""
        self.optimizer.state.clear()
        for g in self.optimizer.param_groups:
            p, s = self.saved[g["name"]]
            g["params"][0] = p
            self.optimizer.state[p] = dict(s)
        return dict(self.params), dict(self.variables), self.optimizer


# ---- the torch chain, in the reference's order ------------------------------------------------------------------------------------

def _group(optimizer, k):
    return [g for g in optimizer.param_groups if g["name"] == k][0]


def torch_remove_points(to_remove, params, variables, optimizer):
    keep = ~to_remove
    for k in MAP_KEYS:
        g = _group(optimizer, k)
        old = g["params"][0]
        s = optimizer.state.get(old, None)
        if s is not None:
            s["exp_avg"], s["exp_avg_sq"] = s["exp_avg"][keep], s["exp_avg_sq"][keep]
            del optimizer.state[old]
        g["params"][0] = torch.nn.Parameter(old[keep].requires_grad_(True))
        if s is not None:
            optimizer.state[g["params"][0]] = s
        params[k] = g["params"][0]
    for k in ("means2D_gradient_accum", "denom", "max_2D_radius", "timestep"):
        variables[k] = variables[k][keep]
    return params, variables


def torch_cat(new, params, optimizer):
    for k, v in new.items():
        g = _group(optimizer, k)
        old = g["params"][0]
        s = optimizer.state.get(old, None)
        if s is not None:
            s["exp_avg"] = torch.cat((s["exp_avg"], torch.zeros_like(v)), dim=0)
            s["exp_avg_sq"] = torch.cat((s["exp_avg_sq"], torch.zeros_like(v)), dim=0)
            del optimizer.state[old]
        g["params"][0] = torch.nn.Parameter(torch.cat((old, v), dim=0).requires_grad_(True))
        if s is not None:
            optimizer.state[g["params"][0]] = s
        params[k] = g["params"][0]
    return params


def torch_build_rotation(q):
    """[n,3,3] from unnormalised quaternions (one stack in place of the reference's nine slice assignments: fewer launches for this route)"""
    r, x, y, z = (q / torch.sqrt((q * q).sum(1, keepdim=True))).unbind(1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), dim=1).reshape(-1, 3, 3)


def torch_prune(params, variables, optimizer, it, cfg):
    to_remove = (torch.sigmoid(params["logit_opacities"]) < cfg["removal_opacity_threshold"]).squeeze()
    if it >= cfg["remove_big_after"]:
        to_remove = torch.logical_or(to_remove, torch.exp(params["log_scales"]).max(dim=1).values > 0.1)
    return torch_remove_points(to_remove, params, variables, optimizer)


def torch_densify(params, variables, optimizer, it, cfg):
    seen = variables["seen"]
    variables["means2D_gradient_accum"][seen] += torch.norm(variables["means2D"].grad[seen, :2], dim=-1)
    variables["denom"][seen] += 1
    grads = variables["means2D_gradient_accum"] / variables["denom"]
    grads[grads.isnan()] = 0.0
    to_clone = torch.logical_and(grads >= cfg["grad_thresh"], torch.max(torch.exp(params["log_scales"]), dim=1).values <= 0.05)
    params = torch_cat({k: params[k][to_clone] for k in MAP_KEYS}, params, optimizer)
    variables["timestep"] = torch.cat((variables["timestep"], torch.zeros((to_clone.sum(),), device=dev)))
    to_split = torch.max(torch.exp(params["log_scales"]), dim=1).values > 0.05
    n = cfg["num_to_split_into"]
    new = {k: params[k][to_split].repeat(n, 1) for k in MAP_KEYS}
    stds = torch.exp(params["log_scales"])[to_split].repeat(n, 1)
    samples = torch.normal(mean=torch.zeros((stds.size(0), 3), device=dev), std=stds)
    rots = torch_build_rotation(params["unnorm_rotations"][to_split]).repeat(n, 1, 1)
    new["means3D"] = new["means3D"] + torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1)
    new["log_scales"] = torch.log(torch.exp(new["log_scales"]) / (0.8 * n))
    params = torch_cat(new, params, optimizer)
    rows = params["means3D"].shape[0]
    variables["timestep"] = torch.cat((variables["timestep"], torch.zeros((to_split.sum() * n,), device=dev)))
    for k in ("means2D_gradient_accum", "denom", "max_2D_radius"):
        variables[k] = torch.zeros(rows, device=dev)
    to_remove = torch.cat((to_split, torch.zeros(n * to_split.sum(), dtype=torch.bool, device=dev)))
    params, variables = torch_remove_points(to_remove, params, variables, optimizer)
    to_remove = (torch.sigmoid(params["logit_opacities"]) < cfg["removal_opacity_threshold"]).squeeze()
    if it >= cfg["remove_big_after"]:
        to_remove = torch.logical_or(to_remove, torch.exp(params["log_scales"]).max(dim=1).values > 0.1 * variables["scene_radius"])
    return torch_remove_points(to_remove, params, variables, optimizer)


OPS = dict(prune=dict(fused=lambda p, v, o: se.prune_gaussians(p, v, o, 1, PRUNE), torch=lambda p, v, o: torch_prune(p, v, o, 1, PRUNE)),
           densify=dict(fused=lambda p, v, o: se.densify(p, v, o, 1, DENSIFY), torch=lambda p, v, o: torch_densify(p, v, o, 1, DENSIFY)))


def call(fn, m):
    return fn(*m.fresh())


def timed(step, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters, 1e3 * (time.perf_counter() - t0) / iters


def compare(routes, iters):
    for step in routes.values():
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    raw = {k: [] for k in routes}
    for _ in range(REPS):
        for k, step in routes.items():
            raw[k].append(timed(step, iters))
    out = {}
    for k, v in raw.items():
        out[k] = {}
        for j, what in enumerate(("event_ms", "wall_ms")):
            s = sorted(t[j] for t in v)
            out[k][what] = dict(median=s[len(s) // 2], min=s[0], max=s[-1])
    return out


def host_syncs(step):
    """synchronisations torch's sync debug mode reports during one call"""
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


def traced_kernels(route, op, iters, P):
    """(kernels, kernels named k_edit_*, mask / statistics kernels of this library) in a kernel trace of a child process that makes `iters` calls"""
    with tempfile.TemporaryDirectory() as tmp:
        subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "t", "--", sys.executable, os.path.abspath(__file__),
                        "--kernels-only", route, "--op", op, "--iters", str(iters), "--size", str(P)],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            raise RuntimeError("rocprofv3 left no kernel trace")
        with open(files[0]) as f:
            names = [row["Kernel_Name"] for row in csv.DictReader(f)]
    return len(names), sum("k_edit_" in n for n in names), sum("k_prune_mask" in n or "k_densify_" in n for n in names)


def launches_per_call(op, P):
    out = {}
    for route in ("fused", "torch"):
        a, b = traced_kernels(route, op, 10, P), traced_kernels(route, op, 20, P)
        out[route] = dict(all=(b[0] - a[0]) / 10.0, edit_kernels=(b[1] - a[1]) / 10.0, mask_kernels=(b[2] - a[2]) / 10.0)
    return out


if "--kernels-only" in sys.argv:
    route, op, iters, P = _opt("--kernels-only"), _opt("--op", "prune"), int(_opt("--iters", "10")), int(_opt("--size", "20000"))
    m = Map(P)
    for _ in range(iters):
        call(OPS[op][route], m)
    torch.cuda.synchronize()
    print(json.dumps(dict(kernels_only=route, op=op, iters=iters, size=P)))
    sys.exit(0)

args = [a for a in sys.argv[1:] if a.endswith(".json")]
sizes = [int(s) for s in _opt("--sizes", "20000,2000000").split(",")]
out = dict(what="one prune_gaussians and one densify (n = 2) on an anisotropic map with Adam state (10 % removed, 5 % cloned, 5 % split), fused map "
                "edit against the torch chain in the reference's order; ms per call, median [min .. max] of 7 alternating repeats after warm-up",
           device=torch.cuda.get_device_name(0), repeats=REPS, cases={})
lines = []
for P in sizes:
    m = Map(P)
    iters = 50 if P <= 100000 else 10
    for op in ("prune", "densify"):
        routes = OPS[op]
        res = compare({k: (lambda fn=fn: call(fn, m)) for k, fn in routes.items()}, iters)
        res["iters"] = iters
        (pa, va), (pb, vb) = call(routes["fused"], m), call(routes["torch"], m)
        res["rows"] = dict(before=P, fused=int(pa["means3D"].shape[0]), torch=int(pb["means3D"].shape[0]))
        # the rows that are no children are identical; the children differ by their samples
        same = pa["means3D"].shape == pb["means3D"].shape and torch.equal(pa["rgb_colors"], pb["rgb_colors"]) and torch.equal(pa["logit_opacities"], pb["logit_opacities"])
        res["rows_agree"] = bool(same and va["timestep"].shape == vb["timestep"].shape and (op == "densify" or torch.equal(pa["means3D"], pb["means3D"])))
        res["host_syncs"] = {k: host_syncs(lambda fn=fn: call(fn, m)) for k, fn in routes.items()}
        for what in ("event_ms", "wall_ms"):
            res[f"torch_over_fused_{what}"] = res["torch"][what]["median"] / res["fused"][what]["median"]
            res[f"fused_range_below_torch_range_{what}"] = res["fused"][what]["max"] < res["torch"][what]["min"]
        out["cases"][f"{op}/{P}"] = res
        tag = f"{op} P={P} ({P} -> {res['rows']['fused']} rows)"
        for k in ("fused", "torch"):
            e, w = res[k]["event_ms"], res[k]["wall_ms"]
            lines.append(f"{tag}  {k:5s}  event {e['median']:.4f} ms [{e['min']:.4f} .. {e['max']:.4f}]   "
                         f"wall {w['median']:.4f} ms [{w['min']:.4f} .. {w['max']:.4f}]   host syncs {res['host_syncs'][k]}")
        lines.append(f"{tag}  torch / fused = {res['torch_over_fused_event_ms']:.2f}x (event), {res['torch_over_fused_wall_ms']:.2f}x (wall); "
                     f"rows agree: {res['rows_agree']}")
    del m
    torch.cuda.empty_cache()
if "--no-trace" not in sys.argv:
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on the PATH: the launch counts cannot be traced (--no-trace leaves them out)")
    for op in ("prune", "densify"):
        n = out["cases"][f"{op}/{sizes[0]}"]["launches_per_call"] = launches_per_call(op, sizes[0])
        lines.append(f"launches per {op} P={sizes[0]} (kernel trace, runs of 10 and 20 calls, difference / 10): "
                     f"fused {n['fused']['all']:.0f} ({n['fused']['edit_kernels']:.0f} of them the map-edit kernels, {n['fused']['mask_kernels']:.0f} the mask / "
                     f"statistics kernels of this library, the rest torch's: mask logic, zeros, the samples), torch {n['torch']['all']:.0f}")
print("\n".join(lines))
print(json.dumps(out))
if args:
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)
    with open(os.path.splitext(args[0])[0] + ".txt", "w") as f:
        f.write("\n".join(lines) + "\n")
