#!/usr/bin/env python3
"""tools/action_plan_bench.py [out.txt] [--size S] [--points P]

What the link between path planning and path evaluation costs on an S x S rooms-and-corridors map (S = 768: 8 x 8 rooms, walls 3 cells
thick, a door 12 cells wide in every wall; the cost field set up once, outside the timing), in one process, the two routes alternating:
  host     PathPlanOps.plan_paths (one kernel, one read) + the reference's action loop restated in NumPy (tests/action_cases.py:
           np_action_planning -- np.linalg.inv, compute_next_campos and atan2 per step, the duplicate filter, the action == 1
           bookkeeping) + evaluate_paths with its host roll-out and inversion, which is the code of the commit before this stage existed.
  device   PathPlanOps.plan_actions (fr_plan_paths + fr_plan_actions, one read) + evaluate_paths(poses_w2c=...) on the poses left on
           the device.
for G = 1, 2, 5, 10, 20 and 40 goals (20 is a planning round's), against a P-Gaussian room shell at 128 x 128.  Every figure: REPS repeats
after a warm-up, a host clock around calls that end in a host read or a device synchronise, median [min .. max].  Launches are counted
from the code (the library's kernels per call); host reads are counted by wrapping Tensor.cpu, synchronisations by torch's sync debug
mode.  Both routes' results are compared before anything is timed."""
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
import action_cases as ac                   # noqa: E402
import plan_cases as pc                     # noqa: E402
from fisher_rast import synthetic           # noqa: E402
from fisher_rast.ops import FisherScorer    # noqa: E402
from fisher_rast.path_eval import evaluate_paths   # noqa: E402
from models.SLAM.utils.recon_helpers import setup_camera   # noqa: E402
from planning.astar import AstarPlanner     # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, WARMUP = 9, 3
S = int(_opt("--size", "768"))
P = int(_opt("--points", "100000"))
STEP = dict(forward_step_size=0.065, turn_angle=10., queue_size=30)
GOAL_COUNTS = (1, 2, 5, 10, 20, 40)
ROOM = 96


def rooms(S, n_goals, room=ROOM, wall=3, door=12, seed=5):
    """the map of tools/path_plan_bench.py, its centre moved so that the start room is the room shell round the origin"""
    label = np.full((S, S), 2)
    for k in range(0, S + 1, room):
        lo, hi = max(k - wall // 2, 0), min(k + wall - wall // 2, S)
        label[lo:hi, :] = 1
        label[:, lo:hi] = 1
    for k in range(room, S, room):
        for mid in range(room // 2, S, room):
            label[k - wall:k + wall, mid - door // 2:mid + door // 2] = 2
            label[mid - door // 2:mid + door // 2, k - wall:k + wall] = 2
    rng = np.random.default_rng(seed)
    start = (room // 2, room // 2)
    goals = []
    while len(goals) < n_goals:
        y, x = int(rng.integers(S)), int(rng.integers(S))
        if label[max(y - 2, 0):y + 3, max(x - 2, 0):x + 3].min() == 2:
            goals.append((y, x))
    centre = float(np.float32((S // 2 - start[1] - 0.5) * 0.05))
    return pc._case(label, start, goals, center=(centre, centre))


def spread(v):
    s = sorted(v)
    return dict(median=s[len(s) // 2], min=s[0], max=s[-1])


def fmt(d):
    return f"{d['median']:.3f} ms [{d['min']:.3f} .. {d['max']:.3f}]"


def wall_ms(step):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    step()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def reads_and_syncs(step):
    """(Tensor.cpu calls, synchronisations torch's debug mode reports) of one call"""
    torch.cuda.synchronize()
    reads = []
    real = torch.Tensor.cpu
    torch.Tensor.cpu = lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1]
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
            torch.Tensor.cpu = real
    return len(reads), sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


c = rooms(S, max(GOAL_COUNTS))
pl = AstarPlanner(device=dev)
pl.grid_dim = np.array([c["W"], c["H"]])
pl._map_center_np = np.asarray(c["center"], np.float64)
pl.map_center = torch.from_numpy(pl._map_center_np).to(dev)
pl.cell_size, pl.cam_height = c["cell"], 0.0
pl.occ_map = torch.from_numpy(c["occ_map"]).to(dev)
pl.setup_start(np.array(c["start"]))

case = dict(name="bench", W=c["W"], H=c["H"], cell=c["cell"], center=c["center"], turn=STEP["turn_angle"], step=STEP["forward_step_size"],
            Q=STEP["queue_size"], cam_height=0.0)
pol = ac.Policy(case)
rng = np.random.default_rng(17)
pos = pol.world_at(np.array([c["start"][1], c["start"][0]]) + 0.5 + rng.uniform(-0.2, 0.2, 2))
agent = ac.yaw_pose(rng.uniform(-np.pi, np.pi), pos[0], 0.0, pos[1])
goal_c2ws = np.zeros((len(c["goals"]), 4, 4), np.float32)
for g, (row, col) in enumerate(c["goals"]):
    w = pol.world_at(np.array([col, row]) + 0.5)
    goal_c2ws[g] = ac.yaw_pose(rng.uniform(-np.pi, np.pi), w[0], 0.0, w[1], np.float32)
case.update(agent=agent, goals=np.array(c["goals"], np.int32), goals_c2w=goal_c2ws)

act = synthetic.activate(synthetic.room_shell(P, seed=7))
cam = setup_camera(128, 128, synthetic.intrinsics(128, 128), np.eye(4), device=dev)
sc = FisherScorer(cam, *(act[k].to(dev) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")))
H_train = torch.zeros((P, sc.columns), device=dev)
sc.run(synthetic.invert_rigid(synthetic.candidate_poses(4, seed=10)).to(dev), out_H=H_train)
EVAL = dict(H_reg_lambda=0.1, acc_H_train_every=5, forward_step_size=STEP["forward_step_size"], turn_angle=STEP["turn_angle"], cam_height=0.0)


def host_route(G):
    sub = dict(case, goals=case["goals"][:G], goals_c2w=goal_c2ws[:G])
    t = [time.perf_counter()]
    paths = pl.plan_paths(sub["goals"]); t.append(time.perf_counter())
    r = ac.np_action_planning(sub, paths_list=paths); t.append(time.perf_counter())
    totals = evaluate_paths(sc, agent, r["path_actions"], [0.0] * len(r["path_actions"]), H_train, **EVAL); t.append(time.perf_counter())
    return r, totals, [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]


def device_route(G):
    t = [time.perf_counter()]
    plan = pl.plan_actions(goal_c2ws[:G], agent, **STEP); t.append(time.perf_counter())
    totals = evaluate_paths(sc, agent, plan.path_actions, [0.0] * len(plan.path_actions), H_train, poses_w2c=plan.kept_w2c(), **EVAL)
    t.append(time.perf_counter())
    return plan, totals, [1e3 * (b - a) for a, b in zip(t[:-1], t[1:])]


lines = [f"action planning + path evaluation on a {S} x {S} rooms-and-corridors map, {P} Gaussians at 128 x 128, {torch.cuda.get_device_name(0)}; queue "
         f"{STEP['queue_size']}, step {STEP['forward_step_size']}, turn {STEP['turn_angle']}; {REPS} repeats after {WARMUP} warm-up calls, the routes alternating, "
         "median [min .. max]"]
out = dict(size=S, points=P, device=torch.cuda.get_device_name(0), by_goals={})
for G in GOAL_COUNTS:
    r, want, _ = host_route(G)
    plan, got, _ = device_route(G)
    same = plan.path_actions == r["path_actions"] and plan.kept_index == r["kept_index"] and r["margin"] > ac.MARGIN
    close = bool(np.allclose(got, want, rtol=1e-5, atol=0, equal_nan=True))
    for _ in range(WARMUP):
        host_route(G), device_route(G)
    hw, dw, hs, ds = [], [], [], []
    for _ in range(REPS):
        hw.append(wall_ms(lambda: hs.append(host_route(G)[2])))
        dw.append(wall_ms(lambda: ds.append(device_route(G)[2])))
    h_reads, h_syncs = reads_and_syncs(lambda: host_route(G))
    d_reads, d_syncs = reads_and_syncs(lambda: device_route(G))
    hs, ds = np.array(hs), np.array(ds)
    kept, actions = len(r["path_actions"]), sum(len(a) for a in r["path_actions"])
    rounds = max([sum(1 for s in range(1, len(a) + 1) if (s + 1) % EVAL["acc_H_train_every"] == 0) for a in r["path_actions"]] + [0])
    res = dict(host_ms=spread(hw), device_ms=spread(dw), host_stage_ms=dict(plan_paths=spread(hs[:, 0]), action_loop=spread(hs[:, 1]), evaluate=spread(hs[:, 2])),
               device_stage_ms=dict(plan_actions=spread(ds[:, 0]), evaluate=spread(ds[:, 1])), host_reads=h_reads, device_reads=d_reads,
               host_syncs=h_syncs, device_syncs=d_syncs, kept=kept, actions=actions, rounds=rounds, same_lists=bool(same), totals_rtol_1e5=close)
    out["by_goals"][G] = res
    lines += [f"G = {G:2d}: {kept} kept paths, {actions} actions, {rounds} scoring rounds; lists equal: {same}; totals within rtol 1e-5: {close}",
              f"  host    {fmt(res['host_ms'])} = plan_paths {fmt(res['host_stage_ms']['plan_paths'])} + action loop {fmt(res['host_stage_ms']['action_loop'])}"
              f" + evaluate_paths {fmt(res['host_stage_ms']['evaluate'])};  {h_reads} host reads, {h_syncs} synchronisations",
              f"  device  {fmt(res['device_ms'])} = plan_actions {fmt(res['device_stage_ms']['plan_actions'])} + evaluate_paths(poses_w2c) "
              f"{fmt(res['device_stage_ms']['evaluate'])};  {d_reads} host reads, {d_syncs} synchronisations",
              f"  host / device = {res['host_ms']['median'] / res['device_ms']['median']:.2f}x"]
faster = [G for G in GOAL_COUNTS if out["by_goals"][G]["device_ms"]["median"] < out["by_goals"][G]["host_ms"]["median"]]
lines += ["library launches before the scoring: host route 1 (k_plan_paths); device route 3 (k_plan_paths, k_action_follow, k_action_keep).  The scoring "
          "rounds launch the same scorer kernels on both routes; per round the host route uploads the inverted poses, the device route gathers them "
          "with one indexing kernel from two small index uploads.",
          f"the device route is faster at G in {faster}" if faster else "the device route is faster at no measured G"]
print("\n".join(lines))
print(json.dumps(out))
args = [a for a in sys.argv[1:] if a.endswith(".txt")]
if args:
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
