"""The object round: the cases, a NumPy restatement of the adv follower, restatements of the object cells and the sorted grid, and
the g++ harness over csrc/fr_action_object_math.h and csrc/fr_goal_math.h.

`np_action_planning_object_adv` restates the loop of NavTester.action_planning_object_adv (tester_gaussians_navigation.py:2385-2496) in
binary64 NumPy, np.linalg.inv and all, the goal poses binary32, written from the reference's text: the padding of a path of one point,
the pruning with its [0, 2] indexing, the early stop, the orientation-only mode, the waypoint skipping, the cap of 200, the keep rule.
Besides its outputs it returns the smallest DECISION MARGIN it met -- how far the nearest comparison was from falling the other way:
    d_goal - 2 step                       the pruning
    d_final - 2.5 step                    near the goal or not
    |dyaw| - radians(turn), dyaw          aligned or not, and the sign that picks action 2 or 3        (the YAW margin)
    d_wp - step                           the stage test
    (||rel_final|| - ||rel_next||) - 0.25 step      the skip
    |ang_wp| - radians(turn)              turn or go forward
Every case has a margin above MARGIN = 1e-9 and a yaw margin above YAW_MARGIN = 1e-6 -- four binary32 ulps at pi, because the goal yaw
is a binary32 value (np.arctan2 of two binary32 scalars) that the library takes as the binary64 atan2 rounded once.  A case that comes
out below gets another seed here, in CASES.
"""
import ctypes
import math
import os

import numpy as np

from action_cases import FILL, Policy, compute_next_campos, ulp32, yaw_pose
import harness_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-9
YAW_MARGIN = 1e-6
Q = 200                            # SAFETY_CAP


# ---- the restatement of the follower ---------------------------------------------------------------------------------------------------

def case_paths(c):
    return [c["paths"][g, :n].astype(np.int64) if n > 0 else np.array([]) for g, n in enumerate(c["lengths"])]


def np_action_planning_object_adv(c, paths_list=None, fixed_prune=False):
    """dict(n_actions [G] (-1: no path), actions (list per goal, None without a path), keep [G], kept_index, path_actions, paths_arr,
    pruned (per goal, None without a path), c2w (per goal [n, 4, 4]), margin, yaw_margin, free_run (the longest run of free stage
    advances), orientation_only / skipped / advanced (per goal: steps of each kind)).  fixed_prune: measure the pruning distance as
    one would expect it, (wx - gx, wz - gz), to show that the reference's indexing matters."""
    policy = Policy(c)
    step, turn_deg = c["step"], c["turn"]
    turn = np.radians(turn_deg)
    POS_TOL_FINAL = 2.5 * step
    YAW_TOL_FINAL = turn
    SKIP_WP_IF_NEAR_GOAL = 2.0 * step
    SKIP_WP_MARGIN = 0.25 * step
    SAFETY_CAP = 200
    paths_list = case_paths(c) if paths_list is None else paths_list
    current_agent_pose = np.asarray(c["agent"], np.float64)
    margin, yaw_margin, free_run = [np.inf], [np.inf], [0]

    def near(v):
        margin[0] = min(margin[0], abs(float(v)))

    def near_yaw(v):
        yaw_margin[0] = min(yaw_margin[0], abs(float(v)))

    def yaw_of_pose(T):
        return np.arctan2(T[0, 2], T[2, 2])

    def angle_wrap(a):
        return np.arctan2(np.sin(a), np.cos(a))

    out = dict(n_actions=[], actions=[], keep=[], kept_index=[], path_actions=[], paths_arr=[], pruned=[], c2w=[], orientation_only=[], skipped=[],
               advanced=[])
    for g, path_grid in enumerate(paths_list):
        pose_np = np.asarray(c["goals_c2w"][g], np.float32)
        finish = np.asarray(c["goals"][g]).astype(np.int64)
        if len(path_grid) == 0:
            for k, v in (("n_actions", -1), ("actions", None), ("keep", 0), ("pruned", None), ("c2w", np.zeros((0, 4, 4))), ("orientation_only", 0),
                         ("skipped", 0), ("advanced", 0)):
                out[k].append(v)
            continue
        if len(path_grid) == 1:
            if not np.array_equal(path_grid[0], finish):
                path_grid = np.concatenate([path_grid, finish[None, :]], axis=0)
            else:
                path_grid = np.concatenate([path_grid, path_grid[0][None, :]], axis=0)
        pruned = []
        goal_world_4 = np.array([pose_np[0, 3], current_agent_pose[1, 3], pose_np[2, 3], 1.0])
        for p in path_grid:
            wpt_world_4 = np.array([*policy.convert_to_world(p + 0.5), current_agent_pose[1, 3], 1.0])
            if fixed_prune:
                d_goal = np.linalg.norm(wpt_world_4[[0, 1]] - goal_world_4[[0, 2]])
            else:
                d_goal = np.linalg.norm((wpt_world_4[[0, 2]] - goal_world_4[[0, 2]]))
            near(d_goal - SKIP_WP_IF_NEAR_GOAL)
            if d_goal > SKIP_WP_IF_NEAR_GOAL:
                pruned.append(p)
        if len(pruned) == 0:
            pruned = [path_grid[0], path_grid[-1]]
        path_grid = np.array(pruned, dtype=np.int32)
        if path_grid.shape[0] < 2:
            path_grid = np.vstack([path_grid, finish[None, :]])

        future_pose = current_agent_pose.copy()
        future_pose[1, 3] = policy.cam_height

        def world_from_grid_cell_center(cell_zy):
            w = policy.convert_to_world(cell_zy + 0.5)
            return np.array([w[0], future_pose[1, 3], w[1], 1.0])

        stage_idx = 1
        stage_goal_w4 = world_from_grid_cell_center(path_grid[stage_idx])
        acts, poses = [], []
        used_steps = 0
        run = 0
        kinds = dict(orientation_only=0, skipped=0, advanced=0)
        while used_steps < SAFETY_CAP:
            final_goal_w4 = np.array([pose_np[0, 3], future_pose[1, 3], pose_np[2, 3], 1.0])
            rel_final = np.linalg.inv(future_pose) @ final_goal_w4
            d_final = np.linalg.norm(rel_final[[0, 2]])
            yaw_now = yaw_of_pose(future_pose)
            yaw_goal = yaw_of_pose(pose_np)
            assert yaw_goal.dtype == np.float32 and yaw_now.dtype == np.float64
            dyaw = angle_wrap(yaw_goal - yaw_now)
            near(d_final - POS_TOL_FINAL)
            if d_final < POS_TOL_FINAL:
                near_yaw(abs(dyaw) - YAW_TOL_FINAL)
            if (d_final < POS_TOL_FINAL) and (abs(dyaw) <= YAW_TOL_FINAL):
                break
            if d_final < POS_TOL_FINAL:
                near_yaw(dyaw)
                act = 2 if dyaw > 0 else 3
                future_pose = compute_next_campos(future_pose, act, step, turn_deg)
                acts.append(act)
                poses.append(future_pose)
                used_steps += 1
                kinds["orientation_only"] += 1
                run = 0
                continue
            rel_wp = np.linalg.inv(future_pose) @ stage_goal_w4
            d_wp = np.linalg.norm(rel_wp[[0, 2]])
            near(d_wp - step)
            if d_wp < step:
                if stage_idx + 1 < len(path_grid):
                    next_wp_w4 = world_from_grid_cell_center(path_grid[stage_idx + 1])
                    rel_next = np.linalg.inv(future_pose) @ next_wp_w4
                    rel_goal = np.linalg.inv(future_pose) @ final_goal_w4
                    diff = np.linalg.norm(rel_goal[[0, 2]]) - np.linalg.norm(rel_next[[0, 2]])
                    near(diff - SKIP_WP_MARGIN)
                    if diff < SKIP_WP_MARGIN:
                        stage_goal_w4 = final_goal_w4
                        stage_idx = len(path_grid) - 1
                        kinds["skipped"] += 1
                    else:
                        stage_idx += 1
                        stage_goal_w4 = world_from_grid_cell_center(path_grid[stage_idx])
                        kinds["advanced"] += 1
                else:
                    stage_goal_w4 = final_goal_w4
                run += 1
                free_run[0] = max(free_run[0], run)
                assert run <= len(path_grid) + 2, "the free stage advances do not end"
                continue
            ang_wp = np.arctan2(rel_wp[0], rel_wp[2])
            near(abs(ang_wp) - turn)
            if ang_wp > turn:
                act = 3
            elif ang_wp < -turn:
                act = 2
            else:
                act = 1
            future_pose = compute_next_campos(future_pose, act, step, turn_deg)
            acts.append(act)
            poses.append(future_pose)
            used_steps += 1
            run = 0
        keep = acts not in out["path_actions"] and len(acts) > 0
        if keep:
            out["path_actions"].append(acts)
            out["kept_index"].append(g)
            out["paths_arr"].append(path_grid)
        for k, v in (("n_actions", len(acts)), ("actions", acts), ("keep", int(keep)), ("pruned", path_grid), ("c2w", np.array(poses).reshape(-1, 4, 4))):
            out[k].append(v)
        for k, v in kinds.items():
            out[k].append(v)
    out["margin"], out["yaw_margin"], out["free_run"] = margin[0], yaw_margin[0], free_run[0]
    return out


# ---- the follower's cases -------------------------------------------------------------------------------------------------------------

def cam_pose(yaw, x, y, z, dtype=np.float64):
    """yaw_pose with columns 0 and 1 negated, as the planner's candidate poses and the agent's own pose are (astar.py:1579-1580): with this
    convention action 2 raises atan2(T[0, 2], T[2, 2]), and the orientation-only mode turns towards the goal's yaw"""
    T = yaw_pose(yaw, x, y, z)
    T[:, 0] *= -1
    T[:, 1] *= -1
    return T.astype(dtype)


def _line(p0, n, dx, dz):
    """n points from p0 = (x, z), advancing by a planner's move (dx, dz)"""
    return [(p0[0] + i * dx, p0[1] + i * dz) for i in range(n)]


def _goal(kind, rng, s, agent_yaw, turn, step, cell):
    """(path points [(x, z)] or a length <= 0, finish (row, col), goal yaw, the goal position's offset from its cell's centre in cells,
    the goal pose's cell (x, z) or None = the finish cell)"""
    sx, sz = s
    yaw = rng.uniform(-math.pi, math.pi)
    off = rng.uniform(-0.3, 0.3, 2)
    per_step = step / cell                                         # cells per forward step
    at = None
    if kind in ("p2", "p63", "p64", "p65", "p130"):                 # along the start's row: the last waypoints lie near the goal
        pts = _line(s, int(kind[1:]), 1, 0)
    elif kind == "pass":                                            # the path runs past the goal's column: waypoints 64 +- 2 steps go, across a chunk
        pts = _line(s, 100, 1, 0)
        at = (sx + 64, sz)
    elif kind == "L":
        a, b = int(rng.integers(10, 16)), int(rng.integers(9, 14))
        pts = [(sx, sz), (sx + a, sz), (sx + a, sz + b)]
    elif kind == "corner":                                          # a corner less than two steps in front of the goal, off the straight way to it
        ps = int(round(per_step))
        pts = [(sx, sz), (sx + 6 * ps, sz), (sx + 9 * ps, sz), (sx + 9 * ps, sz + int(1.8 * ps))]
    elif kind == "moves":
        pts, (x, z) = [(sx, sz)], (sx, sz)
        for _ in range(int(rng.integers(5, 12))):
            dx, dz = [(3, 0), (3, 1), (3, 3), (1, 3), (0, 3)][int(rng.integers(0, 5))]
            x, z = x + dx, z + dz
            pts.append((x, z))
    elif kind == "far":                                             # a list that hits the cap
        pts = [(sx, sz), (sx + int(230 * per_step), sz)]
    elif kind == "one":
        return [(sx, sz)], (sz, sx + 1), yaw, off, None
    elif kind == "one-same":                                        # one point that IS the finish, element-wise: x = row, z = col
        return [(sx, sz)], (sx, sz), yaw, off, None
    elif kind == "one-left":                                        # the end lies at the goal and goes, the start stays: `finish` is appended
        pts = [(sx, sz), (sx + 12, sz)]
    elif kind == "all-pruned":                                      # every waypoint within 2 steps of the goal: [first, last] is left
        pts = [(sx, sz), (sx + 1, sz), (sx + 1, sz + 1)]
        off = rng.uniform(-0.2, 0.2, 2)
    elif kind in ("at-goal+", "at-goal-", "at-goal-empty"):          # reached in position at the start: orientation-only from step 0
        pts = [(sx, sz), (sx + 1, sz)]
        sign = 1 if kind == "at-goal+" else -1
        yaw = agent_yaw + sign * math.radians(turn) * (rng.uniform(0.15, 0.85) if kind == "at-goal-empty" else rng.uniform(2.2, 4.8))
        off = rng.uniform(-0.2, 0.2, 2)
    elif kind == "skip":                                            # the next waypoint lies beside the way: the follower jumps to the goal
        d = int(4 * per_step) + 3
        pts = [(sx, sz), (sx + d, sz), (sx + d, sz + 3 * d), (sx + 3 * d, sz + 3 * d)]
        return pts, (sz + 0, sx + 3 * d), yaw, off, None
    elif kind == "no-skip":                                         # waypoints in a line towards the goal: each one is taken
        d = int(4 * per_step) + 3
        pts = [(sx, sz), (sx + d, sz), (sx + 2 * d, sz), (sx + 3 * d, sz), (sx + 5 * d, sz)]
    elif kind == "none0":
        return 0, (sz + 5, sx + 5), yaw, off, None
    elif kind == "none-1":
        return -1, (sz + 9, sx + 2), yaw, off, None
    else:
        raise ValueError(kind)
    return pts, (pts[-1][1], pts[-1][0]), yaw, off, at


def _case(seed, kinds, W=160, H=160, cell=0.05, center=(0.0, 0.0), turn=10., step=0.065, start=(20, 22), agent_yaw=None, dups=(), slack=1,
          agent_y=1.3):
    """kinds: one per goal; dups: (g, h) pairs -- goal g repeats goal h (same path, same pose).  agent_y: the agent's own height, which
    the pruning measures against the goal's z; "row" puts it at the world z of the start's row, so that goals on that row see their
    near waypoints pruned -- at 1.3 it is so far from any goal's z that nothing is ever pruned."""
    rng = np.random.default_rng(seed)
    c = dict(W=W, H=H, cell=cell, center=tuple(float(np.float32(v)) for v in center), turn=turn, step=step, Q=Q, cam_height=0.4)
    policy = Policy(c)
    pos = policy.world_at(np.array(start) + 0.5 + rng.uniform(-0.2, 0.2, 2))
    agent_yaw = rng.uniform(-math.pi, math.pi) if agent_yaw is None else agent_yaw + rng.uniform(-0.05, 0.05)
    if agent_y == "row":
        agent_y = float(policy.world_at(np.array(start) + 0.5)[1]) + 0.0137
    c["agent"] = cam_pose(agent_yaw, pos[0], agent_y, pos[1])
    c["start"] = start
    goals = [_goal(k, rng, start, agent_yaw, turn, step, cell) for k in kinds]
    for g, h in dups:
        goals[g] = goals[h]
    max_len = max([len(g[0]) for g in goals if not isinstance(g[0], int)] + [1]) + slack
    G = len(goals)
    c["paths"] = np.full((G, max_len, 2), FILL, np.int32)
    c["lengths"] = np.zeros(G, np.int32)
    c["goals"] = np.zeros((G, 2), np.int32)
    c["goals_c2w"] = np.zeros((G, 4, 4), np.float32)
    for g, (pts, finish, yaw, off, at) in enumerate(goals):
        if isinstance(pts, int):
            c["lengths"][g] = pts
        else:
            c["lengths"][g] = len(pts)
            c["paths"][g, :len(pts)] = pts
        c["goals"][g] = finish
        at = np.array([finish[1], finish[0]]) if at is None else np.array(at)
        w = policy.world_at(at + 0.5 + off)
        c["goals_c2w"][g] = cam_pose(yaw, w[0], rng.uniform(0.2, 1.5), w[1], np.float32)
    for g, h in dups:
        c["goals_c2w"][g] = c["goals_c2w"][h]
    c["max_len"] = max_len
    c["kinds"] = list(kinds)
    return c


_MIX = ("L", "p2", "none0", "moves", "one", "at-goal-empty", "none-1", "at-goal+", "all-pruned", "skip", "no-skip", "at-goal-", "one-same", "one-left")

CASES = {
    # name: (seed, arguments of _case)
    "g1": (1, dict(kinds=("L",), turn=10., step=0.065)),
    "lanes": (2, dict(kinds=("p2", "p63", "p64", "p65", "p130", "pass"), turn=30., step=0.25, W=200, H=120, agent_y="row")),   # pruning across chunks
    "one-point": (3, dict(kinds=("one", "one-same", "one"), turn=10., step=0.065, start=(30, 22))),
    "all-pruned": (4, dict(kinds=("all-pruned", "all-pruned"), turn=30., step=0.25, agent_y="row")),
    "one-left": (14, dict(kinds=("one-left", "one-left"), turn=10., step=0.065, agent_y="row")),
    "at-goal": (5, dict(kinds=("at-goal+", "at-goal-", "at-goal-empty", "at-goal-empty"), turn=10., step=0.25, agent_yaw=0.4)),
    "skip": (6, dict(kinds=("skip", "no-skip"), turn=10., step=0.25, W=200, H=200, agent_yaw=1.2)),
    "cap": (7, dict(kinds=("far", "L"), turn=10., step=0.065, W=360, H=64, agent_yaw=1.5)),
    # the agent's height 1.3 is not cam_height and lies more than 3 from the goals' z: (wx - gx, h - gz) is that long whatever the waypoint
    # and nothing is pruned; by (wx - gx, wz - gz) the last waypoints lie within two steps and go
    "height-quirk": (8, dict(kinds=("corner", "L"), turn=30., step=0.25, agent_y=1.3, start=(20, 22))),
    "odd-grid": (10, dict(kinds=_MIX, W=167, H=171, center=(0.37, -1.21), turn=10., step=0.25, start=(9, 13), slack=3, agent_y="row")),
    "g70": (11, dict(kinds=tuple(_MIX[k % len(_MIX)] for k in range(70)), W=231, H=197, center=(-2.5, 0.125), turn=30., step=0.25,
                     dups=((40, 3), (69, 0)), agent_y="row")),
    "all-without-path": (12, dict(kinds=("none0", "none-1", "none0"))),
}
FAMILIES = tuple(CASES)


def make_case(name):
    seed, kw = CASES[name]
    c = _case(seed, **kw)
    c["name"] = name
    return c


# ---- restatements of the object cells and the sorted grid ----------------------------------------------------------------------------------

def occ_uniform(seed, k, j):
    """the ring kernel's counter-based generator (fisher_occ.hip: occ_uniform), float32 in [0, 1)"""
    k = np.asarray(k, np.uint64)
    x = (np.uint64(seed) + np.uint64(0x9E3779B9) * (np.uint64(4) * k + np.uint64(j + 1))) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16); x = (x * np.uint64(0x7feb352d)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15); x = (x * np.uint64(0x846ca68b)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    return (x >> np.uint64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def np_object_cells(W, H, cell, center, points, min_count, max_cells):
    """(cells int32 [min(found, max_cells), 2] = (col, row) in np.where order, counts [found, binned]): discretize_coords in float32,
    clamped, np.unique with counts, a mask, np.where -- build_object_frontiers' own steps; rows with a non-finite x or z left out"""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    ok = np.isfinite(pts[:, 0]) & np.isfinite(pts[:, 2])
    pts = pts[ok]
    cell, cx, cz = np.float32(cell), np.float32(center[0]), np.float32(center[1])
    with np.errstate(over="ignore"):
        col = np.floor((pts[:, 0] - cx) / cell) + np.float32(W - 1) / np.float32(2.0)
        row = np.floor((pts[:, 2] - cz) / cell) + np.float32(H - 1) / np.float32(2.0)
    col = np.clip(col, 0, W - 1).astype(np.int64)                  # the clamp first: a float far outside the map has no int
    row = np.clip(row, 0, H - 1).astype(np.int64)
    found = np.zeros((0, 2), np.int64)
    if len(pts):
        uniq, cnt = np.unique(np.stack([col, row], axis=1), axis=0, return_counts=True)
        mask = np.zeros((H, W), np.uint8)
        uv = uniq[cnt > min_count]
        mask[uv[:, 1], uv[:, 0]] = 1
        found = np.stack(np.where(mask), axis=1)[:, [1, 0]]
    return found[:max_cells].astype(np.int32), [len(found), int(ok.sum())]


def n_theta_of(theta_step_deg):
    """max(1, round(2 pi / deg2rad(step))) as the reference takes it: binary32, round half to even"""
    step_rad = np.deg2rad(np.float32(theta_step_deg))
    return max(1, int(np.round(np.float32(2 * math.pi) / step_rad)))


def np_grid_tables(n_theta, bins, sqrt_area, min_range, radius):
    """(angles, radii) float32: binary64 linspaces rounded once"""
    thetas = np.linspace(0.0, 2 * math.pi, n_theta)
    thetas = thetas[:-1] if len(thetas) > 1 else thetas
    lo, hi = float(np.float32(min_range)), float(np.float32(radius))
    if sqrt_area and bins > 1:
        r = np.sqrt(lo * lo + np.linspace(0.0, 1.0, bins) * (hi * hi - lo * lo))
    else:
        r = np.linspace(lo, hi, bins)
    return thetas.astype(np.float32), r.astype(np.float32)


def np_grid_candidates(W, H, cell, center, centers, K, min_range, radius, n_theta, bins, sqrt_area, cam_height, seed, eroded=None, min_free=40):
    """(c2w float32 [K, 4, 4], keep uint8 [K]) of the sorted grid around float32 centres [n, 2], in float32 NumPy on the kernel's draws"""
    f = np.float32
    thetas, radii = np_grid_tables(n_theta, bins, sqrt_area, min_range, radius)
    R, T = np.meshgrid(radii, thetas, indexing="ij")
    R, T = R.reshape(-1), T.reshape(-1)
    k = np.arange(K)
    R, T = R[k % len(R)], T[k % len(T)]
    centers = np.asarray(centers, f).reshape(-1, 2)
    ci = np.minimum((occ_uniform(seed, k, 2) * f(len(centers))).astype(np.int64), len(centers) - 1)
    c2w = np.zeros((K, 4, 4), f)
    c2w[:, 0, 3] = centers[ci, 0] + R * np.sin(T)
    c2w[:, 1, 3] = f(cam_height)
    c2w[:, 2, 3] = centers[ci, 1] + R * np.cos(T)
    yaw = T + f(np.pi)
    qr, qy = np.cos(yaw / f(2)), np.sin(yaw / f(2))
    norm = np.sqrt(qr * qr + qy * qy)
    qr, qy = qr / norm, qy / norm
    d, o = f(1) - f(2) * (qy * qy), f(2) * (qr * qy)
    c2w[:, 0, 0], c2w[:, 0, 2], c2w[:, 2, 0], c2w[:, 2, 2] = -d, o, o, d              # columns 0 and 1 negated
    c2w[:, 1, 1] = -1
    c2w[:, 3, 3] = 1
    keep = np.ones(K, np.uint8)
    if eroded is not None and int(np.count_nonzero(eroded)) > min_free:
        col = ((c2w[:, 0, 3] - f(center[0])) / f(cell) + f(W // 2)).astype(np.int64)
        row = ((c2w[:, 2, 3] - f(center[1])) / f(cell) + f(H // 2)).astype(np.int64)
        inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
        keep = np.where(inside, eroded[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)] != 0, False).astype(np.uint8)
    return c2w, keep


def cells_to_world(cells, W, H, cell, center):
    """(cell - grid_dim // 2) * cell_size + map_center on the binary32 cell size and centre, in binary64, rounded once"""
    cells = np.asarray(cells, np.int64).reshape(-1, 2)
    half = np.array([W // 2, H // 2])
    return ((cells - half) * float(np.float32(cell)) + np.asarray(center, np.float32).astype(np.float64)).astype(np.float32)


# ---- the g++ harness ------------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_goal_harness", harness_build.EXACT))
    vp, ci, cf, cd, cu = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_uint32
    h.frg_h_object_max.restype = ci
    h.frg_h_plan_object.argtypes = [ci, ci, cd, cf, cf, vp, ci, vp, vp, vp, ci, vp, cd, cd, cd] + [vp] * 9
    h.frg_h_plan_object.restype = None
    h.frg_h_object_cells.argtypes = [ci, ci, cf, cf, cf, vp, ci, ci, vp, ci, vp]
    h.frg_h_object_cells.restype = None
    h.frg_h_tables.argtypes = [ci, ci, ci, cf, cf, vp, vp]
    h.frg_h_tables.restype = None
    h.frg_h_grid.argtypes = [vp, ci, ci, cf, cf, ci, ci, ci, cf, cu, vp]
    h.frg_h_grid.restype = None
    return h


def case_arrays(c):
    return dict(paths=np.ascontiguousarray(c["paths"], np.int32), lengths=np.ascontiguousarray(c["lengths"], np.int32),
                goals=np.ascontiguousarray(c["goals"], np.int32), goals_c2w=np.ascontiguousarray(c["goals_c2w"], np.float32).reshape(-1, 16),
                agent=np.ascontiguousarray(c["agent"], np.float64).reshape(16))


def harness_plan(h, c):
    """dict(actions uint8 [G, 200], n_actions, keep, w2c float32 [G, 200, 4, 4], c2w_xz float64 [G, 200, 2], map_xz int32 [G, 200, 2],
    pruned int32 [G, max_len + 1, 2], pruned_len, bound_hit)"""
    a = case_arrays(c)
    G, L = len(a["lengths"]), c["max_len"] + 1
    out = dict(actions=np.full((G, Q), 0x5A, np.uint8), n_actions=np.zeros(G, np.int32), keep=np.full(G, 0x5A, np.uint8),
               w2c=np.full((G, Q, 4, 4), np.nan, np.float32), c2w_xz=np.full((G, Q, 2), np.nan), map_xz=np.full((G, Q, 2), 0x5A5A5A5A, np.int32),
               pruned=np.full((G, L, 2), 0x5A5A5A5A, np.int32), pruned_len=np.full(G, 0x5A5A5A5A, np.int32), bound_hit=np.full(G, 0x5A5A5A5A, np.int32))
    h.frg_h_plan_object(c["W"], c["H"], c["cell"], c["center"][0], c["center"][1], a["paths"].ctypes.data, c["max_len"], a["lengths"].ctypes.data,
                        a["goals"].ctypes.data, a["goals_c2w"].ctypes.data, G, a["agent"].ctypes.data, c["cam_height"], c["step"], c["turn"],
                        out["actions"].ctypes.data, out["n_actions"].ctypes.data, out["keep"].ctypes.data, out["w2c"].ctypes.data,
                        out["c2w_xz"].ctypes.data, out["map_xz"].ctypes.data, out["pruned"].ctypes.data, out["pruned_len"].ctypes.data,
                        out["bound_hit"].ctypes.data)
    return out


def compare(got, want, c):
    """asserts that `got` (the layout of harness_plan) equals the restatement `want` by the issue's rules; returns the figures"""
    G = len(c["lengths"])
    assert want["margin"] > MARGIN, (c["name"], want["margin"])
    assert want["yaw_margin"] > YAW_MARGIN, (c["name"], want["yaw_margin"])
    assert got["n_actions"].tolist() == want["n_actions"], c["name"]
    assert got["keep"].tolist() == want["keep"], c["name"]
    worst_xz, worst_ulp = 0.0, 0
    policy = Policy(c)
    for g in range(G):
        n = max(want["n_actions"][g], 0)
        assert got["actions"][g, :n].tolist() == (want["actions"][g] or []), (c["name"], g)
        # behind the list and behind the pruned path: the documented zeros
        assert not got["actions"][g, n:].any() and not got["w2c"][g, n:].any() and not got["c2w_xz"][g, n:].any() and not got["map_xz"][g, n:].any()
        m = 0 if want["pruned"][g] is None else len(want["pruned"][g])
        assert got["pruned_len"][g] == m and not got["pruned"][g, m:].any(), (c["name"], g)
        if m:
            assert np.array_equal(got["pruned"][g, :m], want["pruned"][g]), (c["name"], g)
        if n == 0:
            continue
        c2w = want["c2w"][g]
        worst_xz = max(worst_xz, float(np.abs(got["c2w_xz"][g, :n] - c2w[:, [0, 2], 3]).max()))
        worst_ulp = max(worst_ulp, int(ulp32(got["w2c"][g, :n], np.linalg.inv(c2w).astype(np.float32)).max()))
        assert got["map_xz"][g, :n].tolist() == [policy.convert_to_map(p[[0, 2], 3]).tolist() for p in c2w], (c["name"], g)
    assert worst_xz <= 1e-12, (c["name"], worst_xz)
    assert worst_ulp <= 1, (c["name"], worst_ulp)
    return worst_xz, worst_ulp
