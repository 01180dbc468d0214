#!/usr/bin/env python3
"""tools/object_round_bench.py [out.txt] [--size S] [--points P]

What the object round costs before its paths are scored, on an S x S rooms-and-corridors map (S = 768: the map of
tools/action_plan_bench.py), in one process, the two routes alternating:
  follower   host:    PathPlanOps.plan_paths (one kernel, one read) + the loop of NavTester.action_planning_object_adv restated in NumPy
                      (tests/goal_cases.py: np_action_planning_object_adv -- pruning, three to five np.linalg.inv per step, up to 200 actions)
             device:  PathPlanOps.plan_actions_object (fr_plan_paths + fr_plan_actions_object, one read)
  stage      the whole of plan_best_object_path before the scoring: GoalSelectOps.global_object_planning on a P-Gaussian object cloud with a
             stub pose evaluation (the same library code on both routes), setup_start, then the follower by either route.
for G = 1, 20 and 40 goals (20 is a planning round's top-k).  Every figure: REPS repeats after a warm-up, a host clock around calls that end
in a host read or a device synchronise, median [min .. max].  Both routes' lists are compared before anything is timed.  No ratio is promised:
this writes down what is measured."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "fisher-nerf-customized_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np   # noqa: E402
import torch         # noqa: E402
import __graft_entry__ as entry   # noqa: E402

entry.build()
import goal_cases as gc                     # noqa: E402
import plan_cases as pc                     # noqa: E402
from planning.astar import AstarPlanner     # noqa: E402


def _opt(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


dev = torch.device("cuda:0")
REPS, WARMUP = 9, 3
S = int(_opt("--size", "768"))
P = int(_opt("--points", "20000"))
STEP = dict(forward_step_size=0.065, turn_angle=10.)
GOAL_COUNTS = (1, 20, 40)
ROOM = 96


def rooms(S, n_goals, room=ROOM, wall=3, door=12, seed=5):
    """the map of tools/action_plan_bench.py: rooms of 96 cells, walls 3 cells thick, a door 12 cells wide in every wall"""
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


c = rooms(S, max(GOAL_COUNTS))
pl = AstarPlanner(device=dev, sample_view_num_object=138, sample_range_object=1.5, min_range_object=0.4)
pl.grid_dim = np.array([c["W"], c["H"]])
pl._map_center_np = np.asarray(c["center"], np.float64)
pl.map_center = torch.from_numpy(pl._map_center_np).to(dev)
pl.cell_size, pl.cam_height = c["cell"], 0.0
pl.occ_map = torch.from_numpy(c["occ_map"]).to(dev)
pl.cam_pos = np.array(c["start"])
pl.candidate_seed = 3
start_cell = np.array(c["start"])
pl.setup_start(start_cell)

case = dict(name="bench", W=c["W"], H=c["H"], cell=c["cell"], center=c["center"], turn=STEP["turn_angle"], step=STEP["forward_step_size"], Q=gc.Q,
            cam_height=0.0)
pol = gc.Policy(case)
rng = np.random.default_rng(17)
pos = pol.world_at(np.array([c["start"][1], c["start"][0]]) + 0.5 + rng.uniform(-0.2, 0.2, 2))
agent = gc.cam_pose(rng.uniform(-np.pi, np.pi), pos[0], 0.0, pos[1])
goal_c2ws = np.zeros((len(c["goals"]), 4, 4), np.float32)
for g, (row, col) in enumerate(c["goals"]):
    w = pol.world_at(np.array([col, row]) + 0.5)
    goal_c2ws[g] = gc.cam_pose(rng.uniform(-np.pi, np.pi), w[0], 0.0, w[1], np.float32)
case.update(agent=agent, goals=np.array(c["goals"], np.int32), goals_c2w=goal_c2ws, start=(c["start"][1], c["start"][0]))

# the object: P Gaussians over a patch of 8 x 8 cells in the middle of the room next door
patch = pol.world_at(np.array([ROOM + ROOM // 2, ROOM // 2]) + 0.5)
obj = np.zeros((P, 3), np.float32)
obj[:, [0, 2]] = patch + rng.uniform(-0.2, 0.2, (P, 2))
obj[:, 1] = rng.uniform(-0.3, 0.3, P)
obj_points = torch.from_numpy(obj).to(dev)


def pose_eval(poses, random_gaussian_params, criterion=None):
    """a stub in the scorer's place: one small kernel chain and the read the real one ends with"""
    return (10.0 - torch.linalg.norm(poses[:, [0, 2], 3] - poses[:1, [0, 2], 3], dim=1)).cpu(), poses


def host_follower(sub, goals_c2w):
    paths = pl.plan_paths(sub["goals"])
    return gc.np_action_planning_object_adv(dict(sub, goals_c2w=goals_c2w), paths_list=paths)


def stage(G, route):
    pl.TOPK = G
    pl.candidate_seed = 3
    poses, scores, _, _ = pl.global_object_planning(pose_eval, obj_points, None, None, agent_pose=agent[:3, 3])
    order = np.argsort(scores.numpy())[::-1]
    goals = poses.cpu().numpy()[order]
    pl.setup_start(start_cell)
    if route == "device":
        return pl.plan_actions_object(goals, agent, **STEP).path_actions
    cells = np.array([pl._plan_to_map(p[[0, 2], 3])[[1, 0]] for p in goals], np.int32)
    return host_follower(dict(case, goals=cells), goals)["path_actions"]


lines = [f"the object round before its scoring on a {S} x {S} rooms-and-corridors map, an object of {P} Gaussians, {torch.cuda.get_device_name(0)}; "
         f"step {STEP['forward_step_size']}, turn {STEP['turn_angle']}, up to 200 actions; {REPS} repeats after {WARMUP} warm-up calls, the routes "
         "alternating, median [min .. max]"]
out = dict(size=S, points=P, device=torch.cuda.get_device_name(0), by_goals={})
for G in GOAL_COUNTS:
    sub = dict(case, goals=case["goals"][:G])
    r = host_follower(sub, goal_c2ws[:G])
    plan = pl.plan_actions_object(goal_c2ws[:G], agent, **STEP)
    same = plan.path_actions == r["path_actions"] and plan.kept_index == r["kept_index"]
    margins_ok = r["margin"] > gc.MARGIN and r["yaw_margin"] > gc.YAW_MARGIN
    stage_same = stage(G, "device") == stage(G, "host")
    for _ in range(WARMUP):
        host_follower(sub, goal_c2ws[:G]), pl.plan_actions_object(goal_c2ws[:G], agent, **STEP)
    hf, df, hs, ds = [], [], [], []
    for _ in range(REPS):
        hf.append(wall_ms(lambda: host_follower(sub, goal_c2ws[:G])))
        df.append(wall_ms(lambda: pl.plan_actions_object(goal_c2ws[:G], agent, **STEP)))
    for _ in range(REPS):
        hs.append(wall_ms(lambda: stage(G, "host")))
        ds.append(wall_ms(lambda: stage(G, "device")))
    kept, actions = len(r["path_actions"]), sum(len(a) for a in r["path_actions"])
    res = dict(host_follower_ms=spread(hf), device_follower_ms=spread(df), host_stage_ms=spread(hs), device_stage_ms=spread(ds), kept=kept, actions=actions,
               same_lists=bool(same), margins_ok=bool(margins_ok), stage_same_lists=bool(stage_same))
    out["by_goals"][G] = res
    lines += [f"G = {G:2d}: {kept} kept paths, {actions} actions; lists equal: {same} (decision margins above the tests' bars: {margins_ok}); "
              f"the stage's lists equal: {stage_same}",
              f"  follower  host   {fmt(res['host_follower_ms'])}   (plan_paths + the NumPy restatement of the reference loop)",
              f"  follower  device {fmt(res['device_follower_ms'])}   (plan_actions_object: k_plan_paths, k_action_object_follow, k_action_object_keep, one read)",
              f"  stage     host   {fmt(res['host_stage_ms'])}   (global_object_planning + setup_start + the host follower)",
              f"  stage     device {fmt(res['device_stage_ms'])}   (global_object_planning + setup_start + plan_actions_object)"]
print("\n".join(lines))
print(json.dumps(out))
args = [a for a in sys.argv[1:] if a.endswith(".txt")]
if args:
    with open(args[0], "w") as f:
        f.write("\n".join(lines) + "\n")
