"""Action planning: the cases, a NumPy restatement of the reference loop, and the g++ harness over csrc/fr_action_math.h.

`np_action_planning` restates the second half of NavTester.action_planning (tester_gaussians_navigation.py:2246-2330) and the
`action == 1` bookkeeping of plan_best_path (1684-1711) in binary64 NumPy, np.linalg.inv and all, written from the reference's text:
the stage goal at its cell centre, the path of one point that gets `finish` appended in row-col order, the final re-orientation, the
duplicate filter.  Besides its outputs it returns the smallest DECISION MARGIN it met -- how far the nearest comparison was from
falling the other way:
    | ||rel|| - forward_step_size |          the stage test
    | |angle| - radians(turn_angle) |        turn or go forward
    |dyaw| mod turn_angle, and what is left to the next multiple      the number of final turns
    | |dyaw| - 180 |                         the wrap
    |dyaw|                                   the sign that picks action 2 or 3
The reference's decisions are arbitrary on a knife edge, so every case here has a margin above MARGIN (tests assert it before they
compare anything); start position, yaw and goal yaws are drawn from continuous distributions, and a case that comes out below the
margin gets another seed here, in CASES.
"""
import ctypes
import math
import os

import numpy as np
import harness_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
FILL = -7777                       # what stands in `paths` behind a path's end: never a cell


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def compute_next_campos(cam_H, action_id, forward_step_size, turn_angle):
    """models/SLAM/utils/slam_external.py:44-65"""
    next_H = cam_H.copy()
    if action_id == 1:
        next_H[:3, 3] = cam_H[:3, 3] + cam_H[:3, :3] @ np.array([0.0, 0.0, forward_step_size])
    elif action_id in (2, 3):
        a = np.deg2rad(turn_angle)
        s = -np.sin(a) if action_id == 2 else np.sin(a)
        R = np.array([[np.cos(a), 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, np.cos(a)]])
        next_H[:3, :3] = cam_H[:3, :3] @ R
    return next_H


class Policy:
    """the two conversions of the reference's AstarPlanner (planning/astar.py:1372-1381); map_center is binary32 there"""

    def __init__(self, c):
        self.map_center = np.asarray(c["center"], np.float32)
        self.cell_size = c["cell"]
        self.grid_dim = np.array([c["W"], c["H"]])
        self.cam_height = c["cam_height"]

    def convert_to_map(self, coord):
        x = int((coord[0] - self.map_center[0]) / self.cell_size + self.grid_dim[0] // 2)
        z = int((coord[1] - self.map_center[1]) / self.cell_size + self.grid_dim[1] // 2)
        return np.array([x, z])

    def convert_to_world(self, coord):
        return (coord - self.grid_dim / 2) * self.cell_size + self.map_center

    def world_at(self, coord):
        """a position that convert_to_map sends to the (fractional) map coordinate `coord` -- on an odd grid not convert_to_world's:
        the reference subtracts grid_dim / 2 one way and adds grid_dim // 2 the other"""
        return (np.asarray(coord, np.float64) - self.grid_dim // 2) * self.cell_size + self.map_center


def case_paths(c):
    """the case's paths as `planning` returns them: an (M, 2) int array in x-z order, or np.array([])"""
    return [c["paths"][g, :n].astype(np.int64) if n > 0 else np.array([]) for g, n in enumerate(c["lengths"])]


def np_action_planning(c, paths_list=None):
    """dict(n_actions [G] (-1: no path), actions (list per goal, None without a path), keep [G], kept_index, path_actions, paths_arr,
    c2w (per goal [n, 4, 4]), world_path / map_path (per goal, the action == 1 entries), margin)"""
    policy = Policy(c)
    step, turn, Q = c["step"], c["turn"], c["Q"]
    paths_list = case_paths(c) if paths_list is None else paths_list
    current_agent_pose = np.asarray(c["agent"], np.float64)
    margin = [np.inf]

    def near(v):
        margin[0] = min(margin[0], abs(float(v)))

    out = dict(n_actions=[], actions=[], keep=[], kept_index=[], path_actions=[], paths_arr=[], c2w=[], world_path=[], map_path=[])
    for g, paths in enumerate(paths_list):
        pose_np = c["goals_c2w"][g]
        finish = np.asarray(c["goals"][g])
        if len(paths) == 0:
            for k, v in (("n_actions", -1), ("actions", None), ("keep", 0), ("c2w", np.zeros((0, 4, 4))), ("world_path", []), ("map_path", [])):
                out[k].append(v)
            continue
        future_pose = current_agent_pose.copy()
        future_pose[1, 3] = policy.cam_height
        stage_goal_idx = 1
        if len(paths) == 1:
            paths = np.concatenate([paths, finish[None, :]], axis=0)
        stage_goal = paths[stage_goal_idx]
        stage_goal_w = policy.convert_to_world(stage_goal + 0.5)
        stage_goal_w = np.array([stage_goal_w[0], future_pose[1, 3], stage_goal_w[1], 1])
        path_action, poses = [], []
        while len(path_action) < Q:
            rel_pos = np.linalg.inv(future_pose) @ stage_goal_w
            xz_rel_pos = rel_pos[[0, 2]]
            near(np.linalg.norm(xz_rel_pos) - step)
            if np.linalg.norm(xz_rel_pos) < step:
                stage_goal_idx += 1
                if stage_goal_idx == len(paths):
                    angle = np.rad2deg(math.atan2(pose_np[0, 2], pose_np[2, 2])) - np.rad2deg(math.atan2(future_pose[0, 2], future_pose[2, 2]))
                    near(abs(angle) - 180)
                    if abs(angle) > 180:
                        angle = angle - 360 if angle > 0 else angle + 360
                    near(angle)
                    near(abs(angle) % turn)
                    near(turn - abs(angle) % turn)
                    num_actions = int(abs(angle) // turn)
                    for k in range(num_actions):
                        if len(path_action) < Q:
                            action = 2 if angle > 0 else 3
                            future_pose = compute_next_campos(future_pose, action, step, turn)
                            path_action.append(action)
                            poses.append(future_pose)
                        else:
                            break
                    break
                else:
                    stage_goal = paths[stage_goal_idx]
                    stage_goal_w = policy.convert_to_world(stage_goal + 0.5)
                    stage_goal_w = np.array([stage_goal_w[0], future_pose[1, 3], stage_goal_w[1], 1])
                    rel_pos = np.linalg.inv(future_pose) @ stage_goal_w
                    xz_rel_pos = rel_pos[[0, 2]]
            angle = np.arctan2(xz_rel_pos[0], xz_rel_pos[1])
            near(abs(angle) - np.radians(turn))
            if angle > np.radians(turn):
                action = 3
            elif angle < -np.radians(turn):
                action = 2
            else:
                action = 1
            future_pose = compute_next_campos(future_pose, action, step, turn)
            path_action.append(action)
            poses.append(future_pose)
        keep = path_action not in out["path_actions"]
        if keep:
            out["path_actions"].append(path_action)
            out["kept_index"].append(g)
            out["paths_arr"].append(paths)
        world_path = [p[[0, 2], 3] for a, p in zip(path_action, poses) if a == 1]
        for k, v in (("n_actions", len(path_action)), ("actions", path_action), ("keep", int(keep)),
                     ("c2w", np.array(poses).reshape(-1, 4, 4)), ("world_path", world_path), ("map_path", [policy.convert_to_map(w) for w in world_path])):
            out[k].append(v)
    out["margin"] = margin[0]
    return out


# ---- the cases ------------------------------------------------------------------------------------------------------------------------

def yaw_pose(yaw, x, y, z, dtype=np.float64):
    """c2w of a camera at (x, y, z) turned by `yaw` radians about y: atan2(T[0, 2], T[2, 2]) = yaw"""
    T = np.eye(4)
    T[0, 0] = T[2, 2] = math.cos(yaw)
    T[0, 2] = math.sin(yaw)
    T[2, 0] = -math.sin(yaw)
    T[:3, 3] = (x, y, z)
    return T.astype(dtype)


def _goal(kind, rng, s, agent_yaw, turn):
    """(path points [(x, z)] or a length <= 0, finish (row, col), goal yaw) of one goal of a kind, from the start cell s = (x, z)"""
    sx, sz = s
    yaw = rng.uniform(-math.pi, math.pi)
    if kind == "straight":
        d = int(rng.integers(20, 46))
        pts = [(sx, sz), (sx + d, sz)]
    elif kind == "straight-far":
        pts = [(sx, sz), (sx + 60, sz)]
    elif kind == "L":
        a, b = int(rng.integers(8, 16)), int(rng.integers(8, 14))
        pts = [(sx, sz), (sx + a, sz), (sx + a, sz + b)]
    elif kind == "moves":                                         # a chain of the planner's own moves, several stages within one step
        pts, (x, z) = [(sx, sz)], (sx, sz)
        for _ in range(int(rng.integers(4, 12))):
            dx, dz = [(3, 0), (3, 1), (3, 3), (1, 3), (0, 3), (-1, 3)][int(rng.integers(0, 6))]
            x, z = x + dx, z + dz
            pts.append((x, z))
    elif kind == "one":                                           # one point: the end cell is the start's neighbour, `finish` gets appended
        return [(sx, sz)], (sz, sx + 1), yaw
    elif kind == "two-near-empty":                                # two points within one step, the goal's yaw within one turn: no action
        pts = [(sx, sz), (sx + 1, sz)]
        yaw = agent_yaw + math.radians(turn) * rng.uniform(0.15, 0.85) * (1 if rng.random() < 0.5 else -1)
    elif kind == "two-near":
        pts = [(sx, sz), (sx + 1, sz)]
    elif kind == "wrap":                                          # the two yaws differ by more than 180 degrees before the wrap
        pts = [(sx, sz), (sx, sz + 1)]
        yaw = -math.copysign(math.pi - rng.uniform(0.1, 1.2), agent_yaw)
    elif kind == "none0":
        return 0, (sz + 5, sx + 5), yaw
    elif kind == "none-1":
        return -1, (sz + 9, sx + 2), yaw
    else:
        raise ValueError(kind)
    return pts, (pts[-1][1], pts[-1][0]), yaw


def _case(seed, kinds, W=96, H=96, cell=0.05, center=(0.0, 0.0), turn=10., step=0.065, Q=30, start=(20, 22), agent_yaw=None, dups=(), slack=1):
    """kinds: one per goal; dups: (g, h) pairs -- goal g repeats goal h (same path, same pose)"""
    rng = np.random.default_rng(seed)
    c = dict(W=W, H=H, cell=cell, center=tuple(float(np.float32(v)) for v in center), turn=turn, step=step, Q=Q, cam_height=0.4)
    policy = Policy(c)
    off = rng.uniform(-0.2, 0.2, 2)
    pos = policy.world_at(np.array(start) + 0.5 + off)
    agent_yaw = rng.uniform(-math.pi, math.pi) if agent_yaw is None else agent_yaw + rng.uniform(-0.05, 0.05)
    c["agent"] = yaw_pose(agent_yaw, pos[0], 1.3, pos[1])
    c["start"] = start
    goals = [_goal(k, rng, start, agent_yaw, turn) for k in kinds]
    for g, h in dups:
        goals[g] = goals[h]
    max_len = max([len(p) for p, _, _ in goals if not isinstance(p, int)] + [1]) + slack
    G = len(goals)
    c["paths"] = np.full((G, max_len, 2), FILL, np.int32)
    c["lengths"] = np.zeros(G, np.int32)
    c["goals"] = np.zeros((G, 2), np.int32)
    c["goals_c2w"] = np.zeros((G, 4, 4), np.float32)
    for g, (pts, finish, yaw) in enumerate(goals):
        if isinstance(pts, int):
            c["lengths"][g] = pts
        else:
            c["lengths"][g] = len(pts)
            c["paths"][g, :len(pts)] = pts
        c["goals"][g] = finish
        w = policy.world_at(np.array([finish[1], finish[0]]) + 0.5)
        c["goals_c2w"][g] = yaw_pose(yaw, w[0], rng.uniform(0.2, 1.5), w[1], np.float32)
    c["max_len"] = max_len
    c["kinds"] = list(kinds)
    return c


_MIX = ("straight", "L", "none0", "moves", "one", "two-near-empty", "none-1", "two-near", "wrap", "straight-far")

CASES = {
    # name: (seed, arguments of _case)
    "corridor": (1, dict(kinds=("straight",), turn=10., step=0.065, Q=30)),                       # G = 1; longer than Q covers
    "L-turn30": (2, dict(kinds=("L", "L", "moves"), turn=30., step=0.25, Q=30)),                  # G = 3; the long turn, the path walked to its end
    "one-point": (3, dict(kinds=("one", "one", "two-near"), turn=10., step=0.065, Q=30, start=(30, 22))),
    "two-near": (4, dict(kinds=("two-near-empty", "two-near", "two-near-empty", "none0"), turn=30., step=0.25, Q=7)),
    "wrap+": (5, dict(kinds=("wrap", "wrap", "two-near"), turn=10., step=0.065, Q=30, agent_yaw=2.85)),
    "wrap-": (6, dict(kinds=("wrap", "wrap", "two-near"), turn=10., step=0.25, Q=30, agent_yaw=-2.85)),
    "q1": (7, dict(kinds=_MIX, turn=10., step=0.065, Q=1)),
    "q7": (8, dict(kinds=_MIX, turn=30., step=0.065, Q=7)),
    "dedupe": (9, dict(kinds=("straight", "straight-far", "L", "straight", "none0", "two-near-empty", "two-near-empty", "L"),
                       turn=10., step=0.065, Q=7, dups=((3, 0), (7, 2)))),                         # 1 equals 0 by its list, 3 is 0 again
    "odd-grid": (10, dict(kinds=_MIX, W=67, H=71, center=(0.37, -1.21), turn=10., step=0.25, Q=30, start=(9, 13), slack=3)),
    "g70": (11, dict(kinds=tuple(_MIX[k % len(_MIX)] for k in range(70)), W=131, H=97, center=(-2.5, 0.125), turn=30., step=0.25, Q=30,
                     dups=((40, 3), (69, 1)))),
    "all-without-path": (12, dict(kinds=("none0", "none-1", "none0"), Q=7)),
    "q-max": (13, dict(kinds=("moves", "straight-far", "L"), turn=10., step=0.065, Q=128)),
}
FAMILIES = tuple(CASES)


def make_case(name):
    seed, kw = CASES[name]
    c = _case(seed, **kw)
    c["name"] = name
    return c


# ---- the g++ harness ------------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_action_harness", harness_build.EXACT))
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    h.fra_h_max_queue.restype = ci
    h.fra_h_plan.argtypes = [ci, ci, cd, cf, cf, vp, ci, vp, vp, vp, ci, vp, cd, cd, cd, ci, vp, vp, vp, vp, vp, vp]
    h.fra_h_plan.restype = None
    h.fra_h_rollout.argtypes = [vp, vp, vp, ci, ci, cd, cd, vp, vp]
    h.fra_h_rollout.restype = None
    return h


def case_arrays(c):
    """the case's inputs as the contiguous arrays the C ABI takes"""
    return dict(paths=np.ascontiguousarray(c["paths"], np.int32), lengths=np.ascontiguousarray(c["lengths"], np.int32),
                goals=np.ascontiguousarray(c["goals"], np.int32), goals_c2w=np.ascontiguousarray(c["goals_c2w"], np.float32).reshape(-1, 16),
                agent=np.ascontiguousarray(c["agent"], np.float64).reshape(16))


def start_of(c):
    """the pose the lists start from: the agent's, at the camera height"""
    s = np.array(c["agent"], np.float64)
    s[1, 3] = c["cam_height"]
    return s


def harness_plan(h, c):
    """dict(actions uint8 [G, Q], n_actions, keep, w2c float32 [G, Q, 4, 4], c2w_xz float64 [G, Q, 2], map_xz int32 [G, Q, 2])"""
    a = case_arrays(c)
    G, Q = len(a["lengths"]), c["Q"]
    out = dict(actions=np.full((G, Q), 0x5A, np.uint8), n_actions=np.zeros(G, np.int32), keep=np.full(G, 0x5A, np.uint8),
               w2c=np.full((G, Q, 4, 4), np.nan, np.float32), c2w_xz=np.full((G, Q, 2), np.nan), map_xz=np.full((G, Q, 2), 0x5A5A5A5A, np.int32))
    h.fra_h_plan(c["W"], c["H"], c["cell"], c["center"][0], c["center"][1], a["paths"].ctypes.data, c["max_len"], a["lengths"].ctypes.data,
                 a["goals"].ctypes.data, a["goals_c2w"].ctypes.data, G, a["agent"].ctypes.data, c["cam_height"], c["step"], c["turn"], Q,
                 out["actions"].ctypes.data, out["n_actions"].ctypes.data, out["keep"].ctypes.data, out["w2c"].ctypes.data,
                 out["c2w_xz"].ctypes.data, out["map_xz"].ctypes.data)
    return out


def harness_rollout(h, start, actions, n_actions, step, turn):
    """(w2c float32 [G, Q, 4, 4], c2w float64 [G, Q, 4, 4])"""
    actions = np.ascontiguousarray(actions, np.uint8)
    n_actions = np.ascontiguousarray(n_actions, np.int32)
    G, Q = actions.shape
    start = np.ascontiguousarray(start, np.float64).reshape(16)
    w2c, c2w = np.full((G, Q, 4, 4), np.nan, np.float32), np.full((G, Q, 4, 4), np.nan)
    h.fra_h_rollout(start.ctypes.data, actions.ctypes.data, n_actions.ctypes.data, G, Q, step, turn, w2c.ctypes.data, c2w.ctypes.data)
    return w2c, c2w


def ulp32(a, b):
    """the distance in binary32 ulps between two float32 arrays (both finite)"""
    def key(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def compare(got, want, c):
    """asserts that `got` (the layout of harness_plan) equals the restatement `want` by the issue's rules; returns the figures"""
    G, Q = len(c["lengths"]), c["Q"]
    assert want["margin"] > MARGIN, (c["name"], want["margin"])
    assert got["n_actions"].tolist() == want["n_actions"], c["name"]
    assert got["keep"].tolist() == want["keep"], c["name"]
    worst_xz, worst_ulp = 0.0, 0
    for g in range(G):
        n = max(want["n_actions"][g], 0)
        assert got["actions"][g, :n].tolist() == (want["actions"][g] or []), (c["name"], g)
        # behind the list: the documented zeros
        assert not got["actions"][g, n:].any() and not got["w2c"][g, n:].any() and not got["c2w_xz"][g, n:].any() and not got["map_xz"][g, n:].any()
        if n == 0:
            continue
        c2w = want["c2w"][g]
        worst_xz = max(worst_xz, float(np.abs(got["c2w_xz"][g, :n] - c2w[:, [0, 2], 3]).max()))
        worst_ulp = max(worst_ulp, int(ulp32(got["w2c"][g, :n], np.linalg.inv(c2w).astype(np.float32)).max()))
        fwd = [k for k in range(n) if want["actions"][g][k] == 1]
        assert got["map_xz"][g, fwd].tolist() == [m.tolist() for m in want["map_path"][g]], (c["name"], g)
        policy = Policy(c)
        assert got["map_xz"][g, :n].tolist() == [policy.convert_to_map(p[[0, 2], 3]).tolist() for p in c2w], (c["name"], g)
    assert worst_xz <= 1e-12, (c["name"], worst_xz)
    assert worst_ulp <= 1, (c["name"], worst_ulp)
    return worst_xz, worst_ulp
