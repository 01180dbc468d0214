#!/usr/bin/env python3
"""tools/path_plan_bench.py [out.txt] [--size S] [--no-best-first]

What the action-planning stage (PathPlanOps.setup_start + plan_paths: fr_plan_grid, fr_occ_freespace, fr_plan_tiers, fr_plan_field,
fr_plan_paths) costs on an S x S rooms-and-corridors map (S = 768: 8 x 8 rooms, walls 3 cells thick, a door 12 cells wide in every
wall) with 20 goals, against two baselines in the same run:
  best-first   the reference-order restatement (tests/plan_cases.py: BestFirst, with np_grid and the tiers): the structure the
               reference executes -- a heapq search per goal, capped at 10^4 expansions, interpreted.  One run (it takes long).
  dijkstra     the g++ harness (tests/harness/fr_plan_harness.cpp) on one core: grid, tiers, a plain Dijkstra over the move table,
               the paths.  The honest CPU alternative.  The map, the free space and the goals would have to come down for it.
Device times: REPS repeats after a warm-up, each a host clock around the call ending in a device synchronise (setup_start reads the
device itself, so wall time is what a planning round waits for) and a pair of events round the same call; median [min .. max].
Rounds, launches and host reads per call are the library's own counts (plan_stats) and torch's sync debug mode."""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
import plan_cases as pc                     # noqa: E402
from planning.astar import AstarPlanner     # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, WARMUP, GOALS = 9, 3, 20
S = int(_opt("--size", "768"))


def rooms(S, room=96, wall=3, door=12, seed=5):
    label = np.full((S, S), 2)
    for k in range(0, S + 1, room):
        lo, hi = max(k - wall // 2, 0), min(k + wall - wall // 2, S)
        label[lo:hi, :] = 1
        label[:, lo:hi] = 1
    for k in range(room, S, room):                      # a door in the middle of every inner wall segment
        for mid in range(room // 2, S, room):
            label[k - wall:k + wall, mid - door // 2:mid + door // 2] = 2
            label[mid - door // 2:mid + door // 2, k - wall:k + wall] = 2
    rng = np.random.default_rng(seed)
    start = (room // 2, room // 2)
    goals = []
    while len(goals) < GOALS:
        y, x = int(rng.integers(S)), int(rng.integers(S))
        if label[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].min() == 2:
            goals.append((y, x))
    return pc._case(label, start, goals)


def spread(v):
    s = sorted(v)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def fmt(d):
    return f"{d['median']:.3f} ms [{d['min']:.3f} .. {d['max']:.3f}]"


def timed(step):
    """(wall ms, event ms) of one call"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    step()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0), a.elapsed_time(b)


def host_syncs(step):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


c = rooms(S)
p = AstarPlanner(device=dev)
p.grid_dim = np.array([c["W"], c["H"]])
p._map_center_np = np.asarray(c["center"], np.float64)
p.map_center = torch.from_numpy(p._map_center_np).to(dev)
p.cell_size, p.cam_height = c["cell"], c["cam_height"]
p.occ_map = torch.from_numpy(c["occ_map"]).to(dev)
start, goals = np.array(c["start"]), np.array(c["goals"])

steps = dict(setup_start=lambda: p.setup_start(start), plan_paths=lambda: p.plan_paths(goals))
res = {}
for name, step in steps.items():
    for _ in range(WARMUP):
        step()
    runs = [timed(step) for _ in range(REPS)]
    res[name] = dict(wall_ms=spread([r[0] for r in runs]), event_ms=spread([r[1] for r in runs]), host_syncs=host_syncs(step))
stats = dict(p.plan_stats)
paths = p.plan_paths(goals)
free = p.free_space_np
occ = p.occ_map_np

# the field alone, through the C ABI on the planner's own buffers
import ctypes                               # noqa: E402
from fisher_rast import _lib                # noqa: E402
lib = _lib.load()
plan, cfg = p._plan, p._plan["cfg"]
need = lib.fr_plan_workspace_bytes(ctypes.byref(cfg))
status = torch.zeros((4,), dtype=torch.int32, device=dev)
counts = (ctypes.c_int32 * 2)()
field_only = lambda: _lib.check(lib.fr_plan_field(ctypes.byref(cfg), plan["tiers"].data_ptr(), int(start[0]), int(start[1]), plan["field"].data_ptr(),
                                                  status.data_ptr(), ctypes.byref(counts), p._plan_ws.data_ptr(), need, p._stream()), "fr_plan_field")
for _ in range(WARMUP):
    field_only()
res["fr_plan_field"] = dict(wall_ms=spread([timed(field_only)[0] for _ in range(REPS)]))

# dijkstra: the g++ harness on one core, on the free space the device built
h = pc.build_harness()
cc = dict(c, free=free)
cpu = {k: [] for k in ("grid", "tiers", "field", "paths")}
for _ in range(3):
    t = [time.perf_counter()]
    h_occ, _ = pc.harness_grid(h, cc); t.append(time.perf_counter())
    h_tiers = pc.harness_tiers(h, free); t.append(time.perf_counter())
    h_field, _ = pc.harness_field(h, h_tiers, c["start"]); t.append(time.perf_counter())
    hp, hl = pc.harness_paths(h, h_field, h_occ, c["start"], c["goals"], True, max_len=4096); t.append(time.perf_counter())
    for k, a, b in zip(cpu, t[:-1], t[1:]):
        cpu[k].append(1e3 * (b - a))
cpu = {k: spread(v) for k, v in cpu.items()}
same_field = bool(np.array_equal(p._plan_read(plan["field"]).view(np.uint64), h_field))
same_paths = all(np.array_equal(a.reshape(-1, 2), hp[k, :hl[k]]) for k, a in enumerate(paths))

lines = [f"path planning on a {S} x {S} rooms-and-corridors map, {GOALS} goals, {torch.cuda.get_device_name(0)}; {REPS} repeats after {WARMUP} warm-up calls, "
         "median [min .. max]",
         f"setup_start (grid, free space, tiers, field)  wall {fmt(res['setup_start']['wall_ms'])}   events {fmt(res['setup_start']['event_ms'])}",
         f"  of which fr_plan_field alone               wall {fmt(res['fr_plan_field']['wall_ms'])}",
         f"plan_paths ({GOALS} goals, shortcut on)           wall {fmt(res['plan_paths']['wall_ms'])}   events {fmt(res['plan_paths']['event_ms'])}",
         f"field: {stats['rounds']} rounds changed something, {stats['rounds_launched']} launched (cap {lib.fr_plan_round_cap(ctypes.byref(cfg))}), "
         f"{stats['convergence_reads']} convergence reads; {int((free != 0).sum())} free cells, {sum(len(a) > 0 for a in paths)} of {GOALS} goals reached, "
         f"longest path {max(len(a) for a in paths)} points after the shortcut",
         f"launches per setup_start: 2 (grid) + 10 (fr_occ_freespace) + 1 (tiers) + 2 + {stats['rounds_launched']} (field) kernels and 5 memsets; per plan_paths: 1",
         f"host synchronisations per call (torch's sync debug mode sees the tensor reads, not the library's own): setup_start "
         f"{res['setup_start']['host_syncs']} + {stats['convergence_reads']} convergence reads in the library, plan_paths {res['plan_paths']['host_syncs']}",
         f"dijkstra (g++ harness, one core): grid {fmt(cpu['grid'])}, tiers {fmt(cpu['tiers'])} (brute force), field {fmt(cpu['field'])}, "
         f"paths {fmt(cpu['paths'])}",
         f"device field equals the harness's word for word: {same_field}; paths equal: {same_paths}",
         f"dijkstra field / fr_plan_field = {cpu['field']['median'] / res['fr_plan_field']['wall_ms']['median']:.2f}x; "
         f"dijkstra (grid + tiers + field + paths) / (setup_start + plan_paths) = "
         f"{sum(v['median'] for v in cpu.values()) / (res['setup_start']['wall_ms']['median'] + res['plan_paths']['wall_ms']['median']):.2f}x"]
out = dict(size=S, goals=GOALS, device=torch.cuda.get_device_name(0), gpu=res, stats=stats, dijkstra_ms=cpu, same_field=same_field, same_paths=same_paths)

if "--no-best-first" not in sys.argv:
    t0 = time.perf_counter()
    b_occ, _ = pc.np_grid(cc)
    bf = pc.BestFirst(b_occ, free, c["start"])
    t1 = time.perf_counter()
    found = sum(len(bf.planning(g)) > 0 for g in c["goals"])
    t2 = time.perf_counter()
    total = 1e3 * (t2 - t0)
    out["best_first_ms"] = dict(grid_and_tiers=1e3 * (t1 - t0), search=1e3 * (t2 - t1), found=found)
    lines.append(f"best-first (reference-order restatement, interpreted, one run): grid and tiers {1e3 * (t1 - t0):.0f} ms, {GOALS} searches "
                 f"{1e3 * (t2 - t1):.0f} ms, {found} of {GOALS} goals found within the cap of 10^4 expansions")
    lines.append(f"best-first / (setup_start + plan_paths) = "
                 f"{total / (res['setup_start']['wall_ms']['median'] + res['plan_paths']['wall_ms']['median']):.0f}x")
print("\n".join(lines))
print(json.dumps(out))
args = [a for a in sys.argv[1:] if a.endswith(".txt")]
if args:
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
