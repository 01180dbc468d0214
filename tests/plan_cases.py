"""The path planner's test material (csrc/fr_plan_math.h, csrc/fr_plan.hip, planning/astar.py: PathPlanOps).

NumPy / heapq restatements, written from the description of the cost model and not from the header:
    np_grid, np_tiers            the planning grid (occ_map_np) and the collision tiers
    np_field                     (a) Dijkstra over the move table with binary32 sums, (b) the parent as the tight predecessor with the
                                 smallest raster index, packed as (cost bits) << 32 | parent
    np_paths                     (c) the goal rule, the walk over the parents and the shortcut loop with the 3.5-cell band
    BestFirst                    (d) the reference's search in its own order (heap key, tuple tie-breaks, relaxation test, the cap of
                                 10^4 expansions, the tree kept from goal to goal), for the dominance property only
and the map families the tests run on.  Cells are (row, col) = (y, x); a family is a dict with the keys of `_case`."""
import ctypes
import heapq
import os

import numpy as np
import harness_build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# astar.py:1641-1682: the displacement and the three path cells of the 16 moves, as (dy, dx)
MOVES = [(-3, 0), (-3, 1), (-3, 3), (-1, 3), (0, 3), (3, 0), (3, 1), (3, 3), (1, 3), (-3, -1), (-3, -3), (-1, -3), (0, -3), (3, -1), (3, -3), (1, -3)]
PATHS = [
    [(-1, 0), (-2, 0), (-3, 0)], [(-1, 0), (-2, 1), (-3, 1)], [(-1, 1), (-2, 2), (-3, 3)], [(0, 1), (-1, 2), (-1, 3)], [(0, 1), (0, 2), (0, 3)],
    [(1, 0), (2, 0), (3, 0)], [(1, 0), (2, 1), (3, 1)], [(1, 1), (2, 2), (3, 3)], [(0, 1), (1, 2), (1, 3)],
    [(-1, 0), (-2, -1), (-3, -1)], [(-1, -1), (-2, -2), (-3, -3)], [(0, -1), (-1, -2), (-1, -3)], [(0, -1), (0, -2), (0, -3)],
    [(1, 0), (2, -1), (3, -1)], [(1, -1), (2, -2), (3, -3)], [(0, -1), (1, -2), (1, -3)]]
UNREACHED = np.uint64(0xFFFFFFFFFFFFFFFF)
STATUS_WORDS = 4


def corridor(m):
    """the nine cells of move m relative to the cell it leaves: rows 0-8 of the table widened by +-1 in x, rows 9-15 by +-1 in y"""
    wy, wx = (0, 1) if m < 9 else (1, 0)
    return PATHS[m] + [(dy + wy, dx + wx) for dy, dx in PATHS[m]] + [(dy - wy, dx - wx) for dy, dx in PATHS[m]]


def move_length(m):
    dy, dx = MOVES[m]
    return np.float32(np.sqrt(np.float64(dy * dy + dx * dx)))


# ---- restatements ---------------------------------------------------------------------------------------------------------------

def cell_of_axis(v, centre, cell, dim):
    """fr_occ_cells_of's rule along one axis without its clamp: (index, inside)"""
    b = np.floor((np.asarray(v, np.float32) - np.float32(centre)) / np.float32(cell)) + np.float32(dim - 1) / np.float32(2.0)
    inside = (b > -1) & (b < dim)
    return np.where(inside, b, 0).astype(np.int64), inside


def np_grid(c):
    """(occ_plan uint8 [H, W], status [4])"""
    H, W = c["H"], c["W"]
    occ = np.argmax(c["occ_map"], axis=0) == 1
    binned = 0
    if c["points"] is not None and len(c["points"]):
        p = np.asarray(c["points"], np.float32)
        lo, hi = np.float32(c["cam_height"]) - np.float32(1.0), np.float32(c["cam_height"])
        p = p[(p[:, 1] >= lo) & (p[:, 1] <= hi)]
        col, okx = cell_of_axis(p[:, 0], c["center"][0], c["cell"], W)
        row, okz = cell_of_axis(p[:, 2], c["center"][1], c["cell"], H)
        keep = okx & okz
        counts = np.zeros((H, W), np.int64)
        np.add.at(counts, (row[keep], col[keep]), 1)
        binned = int(keep.sum())
        occ = occ | (counts > 50)
    pad = np.pad(occ, 1)
    dil = np.zeros((H, W), bool)
    for dy in range(3):
        for dx in range(3):
            dil |= pad[dy:dy + H, dx:dx + W]
    sy, sx = c["start"]
    dil[sy, sx] = False
    ring = int(dil[max(sy - 1, 0):sy + 2, max(sx - 1, 0):sx + 2].sum())
    return dil.astype(np.uint8), np.array([ring, binned, 0, 0], np.int32)


def np_distance(free):
    """L1 distance to the nearest non-free cell inside the grid, capped at 21: 21 rounds of the 4-neighbour relaxation"""
    d = np.where(np.asarray(free) != 0, 21, 0).astype(np.int64)
    for _ in range(21):
        p = np.pad(d, 1, constant_values=21)
        d = np.minimum(d, np.minimum(np.minimum(p[:-2, 1:-1], p[2:, 1:-1]), np.minimum(p[1:-1, :-2], p[1:-1, 2:])) + 1)
    return np.minimum(d, 21)


def np_cell_cost(free):
    """(free bool [H, W], cost int [H, W] in {0, 4, 8, 12})"""
    d = np_distance(free)
    cost = np.select([d <= 5, d <= 10, d <= 20], [12, 8, 4], 0)
    return np.asarray(free) != 0, cost


def np_tiers(free):
    f, cost = np_cell_cost(free)
    return np.where(f, 1 | ((cost // 4) << 1), 0).astype(np.uint8)


def move_weights(free):
    """(valid bool [16, H, W], weight float32 [16, H, W], collision int [16, H, W]) of the move m LEAVING each cell"""
    f, cost = np_cell_cost(free)
    H, W = f.shape
    R = 4
    fp, cp = np.pad(f, R), np.pad(cost, R)
    valid, weight, collision = np.ones((16, H, W), bool), np.zeros((16, H, W), np.float32), np.zeros((16, H, W), np.int64)
    for m in range(16):
        total = np.zeros((H, W), np.int64)
        for dy, dx in corridor(m):
            valid[m] &= fp[R + dy:R + dy + H, R + dx:R + dx + W]
            total += cp[R + dy:R + dy + H, R + dx:R + dx + W]
        weight[m] = move_length(m) + total.astype(np.float32)
        collision[m] = total
    return valid, weight, collision


def np_field(free, start):
    """packed field uint64 [H, W]"""
    f = np.asarray(free) != 0
    H, W = f.shape
    valid, weight, _ = move_weights(free)
    g = np.full((H, W), np.inf, np.float32)
    sy, sx = start
    if f[sy, sx]:
        g[sy, sx] = 0
        heap, done = [(0.0, sy, sx)], np.zeros((H, W), bool)
        while heap:
            gu, y, x = heapq.heappop(heap)
            if done[y, x]:
                continue
            done[y, x] = True
            for m in range(16):
                if valid[m, y, x]:
                    cand = np.float32(g[y, x] + weight[m, y, x])
                    vy, vx = y + MOVES[m][0], x + MOVES[m][1]
                    if cand < g[vy, vx]:
                        g[vy, vx] = cand
                        heapq.heappush(heap, (float(cand), vy, vx))
    # (b) the tight predecessor with the smallest raster index
    parent = np.full((H, W), np.iinfo(np.int64).max, np.int64)
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    for m in range(16):
        dy, dx = MOVES[m]
        ys, xs = np.nonzero(valid[m] & np.isfinite(g))
        vy, vx = ys + dy, xs + dx
        tight = (g[ys, xs] + weight[m, ys, xs]).astype(np.float32) == g[vy, vx]
        np.minimum.at(parent, (vy[tight], vx[tight]), idx[ys[tight], xs[tight]])
    if f[sy, sx]:
        parent[sy, sx] = sy * W + sx
    reached = np.isfinite(g)
    assert (parent[reached] < H * W).all()
    bits = np.where(reached, g, 0).astype(np.float32).view(np.uint32).astype(np.uint64)
    return np.where(reached, (bits << np.uint64(32)) | np.where(reached, parent, 0).astype(np.uint64), UNREACHED)


def field_cost(field):
    """float32 [H, W], -1 where unreached"""
    bits = (np.asarray(field) >> np.uint64(32)).astype(np.uint32)
    return np.where(field == UNREACHED, np.float32(-1), bits.view(np.float32))


def segment_clear(occ, a, b):
    """a, b: (y, x).  True when no occupied cell's centre lies within 3.5 cells of the segment between the two cell centres"""
    H, W = occ.shape
    y0, y1 = max(min(a[0], b[0]) - 4, 0), min(max(a[0], b[0]) + 4, H - 1)
    x0, x1 = max(min(a[1], b[1]) - 4, 0), min(max(a[1], b[1]) + 4, W - 1)
    py, px = np.mgrid[y0:y1 + 1, x0:x1 + 1].astype(np.int64)
    aby, abx, apy, apx = int(b[0] - a[0]), int(b[1] - a[1]), py - a[0], px - a[1]
    ab2, dot = aby * aby + abx * abx, apy * aby + apx * abx
    t = np.clip(dot, 0, ab2)                                   # the projection, clamped to the segment, times |ab|^2
    # |ap - t/ab2 ab|^2 <= 3.5^2, times 4 ab2^2 (ab2 = 0: the point a itself)
    if ab2 == 0:
        inside = 4 * (apy * apy + apx * apx) <= 49
    else:
        qy, qx = apy * ab2 - t * aby, apx * ab2 - t * abx
        inside = 4 * (qy * qy + qx * qx) <= 49 * ab2 * ab2
    return not bool((inside & (occ[y0:y1 + 1, x0:x1 + 1] != 0)).any())


def np_paths(field, occ_plan, start, goals, shortcut):
    """list of (M, 2) int arrays in (x, z) order; an empty array where there is no path"""
    H, W = occ_plan.shape
    cost = field_cost(field)
    out = []
    for gy, gx in goals:
        if not (0 <= gy < H and 0 <= gx < W) or occ_plan[gy, gx]:
            out.append(np.zeros((0, 2), np.int64))
            continue
        cand = [(cost[y, x], y * W + x) for y in range(max(gy - 1, 0), min(gy + 2, H)) for x in range(max(gx - 1, 0), min(gx + 2, W)) if cost[y, x] >= 0]
        if not cand or min(cand)[1] == start[0] * W + start[1]:
            out.append(np.zeros((0, 2), np.int64))
            continue
        chain = [min(cand)[1]]
        while chain[-1] != start[0] * W + start[1]:
            chain.append(int(field.reshape(-1)[chain[-1]] & np.uint64(0xFFFFFFFF)))
        pts = [(i // W, i % W) for i in chain[::-1]]
        if shortcut:
            sc, k = [pts[0], pts[1]], 1
            for i in range(2, len(pts) - 1):
                if segment_clear(occ_plan, sc[k - 1], pts[i]):
                    sc[k] = pts[i]
                else:
                    sc.append(pts[i])
                    k += 1
            sc.append(pts[-1])
            pts = sc
        out.append(np.array([(x, y) for y, x in pts], np.int64))
    return out


class BestFirst:
    """(d) astar.py:1591-1747 in its own order, on the same grid, free space and tiers.  planning(goal) returns the cells (y, x) of
    the path, start first, or []; `direction` is the reference's planning_direction (cost, parent y, parent x, collision cost)."""

    def __init__(self, occ_plan, free, start):
        self.occ, self.free = np.asarray(occ_plan), (np.asarray(free) != 0).astype(np.uint8)
        self.valid, _, self.collision = move_weights(free)             # a move's nine cells inside and free; their summed tier costs
        H, W = self.occ.shape
        self.start = start
        self.direction = np.ones((H, W, 4)) * -1
        self.direction[start[0], start[1]] = [0, start[0], start[1], 0]

    def planning(self, goal):
        H, W = self.occ.shape
        pd = self.direction
        goal = np.array(goal)
        if self.occ[goal[0], goal[1]]:
            return []
        to_goal = np.ones((H, W), np.float32) * -1
        vy, vx = np.where(pd[..., 1] >= 0)
        to_goal[vy, vx] = np.linalg.norm([vy - goal[0], vx - goal[1]], axis=0)
        searched = (pd[..., 1] >= 0).astype(np.uint8)
        p = np.pad(searched, 1, constant_values=1)                # cv2.erode: cells outside do not constrain
        eroded = np.ones((H, W), np.uint8)
        for dy in range(3):
            for dx in range(3):
                eroded &= p[dy:dy + H, dx:dx + W]
        fy, fx = np.where((searched - eroded) * self.free > 0)
        heap = [(to_goal[y, x], y, x) for y, x in zip(fy, fx)]
        heapq.heapify(heap)
        it = 0
        while it < 1e4:
            if not heap:
                break
            _, cy, cx = heapq.heappop(heap)
            cur = np.array([cy, cx])
            if np.max(abs(cur - goal)) < 2:
                goal = cur
                break
            for m in range(16):
                if not self.valid[m, cy, cx]:
                    continue
                n = (cy + MOVES[m][0], cx + MOVES[m][1])
                dist_cost = pd[cy, cx, 0] + np.linalg.norm(np.array(n) - cur)
                collision = pd[cy, cx, 3] + float(self.collision[m, cy, cx])
                if pd[n[0], n[1], 0] < 0 or pd[n[0], n[1], 0] + pd[n[0], n[1], 3] > dist_cost + collision:
                    pd[n[0], n[1]] = [dist_cost, cy, cx, collision]
                    to_goal[n[0], n[1]] = np.linalg.norm(np.array(n) - goal)
                    heapq.heappush(heap, (to_goal[n[0], n[1]] + collision, n[0], n[1]))
            it += 1
        if pd[goal[0], goal[1], 0] < 0:
            return []
        path = [(int(goal[0]), int(goal[1]))]
        while True:
            py, px = pd[path[-1][0], path[-1][1], 1:3].astype(np.int32)
            if (py, px) == path[-1]:
                break
            path.append((int(py), int(px)))
        return [] if len(path) == 1 else path[::-1]

    def tree_costs32(self, weights):
        """{cell: the binary32 sum of the move weights from the start over the tree as it stands} for every reached cell"""
        valid, weight = weights[:2]
        done = {tuple(self.start): np.float32(0)}
        ys, xs = np.where(self.direction[..., 1] >= 0)
        for cell in zip(ys.tolist(), xs.tolist()):
            chain = [cell]
            while chain[-1] not in done:
                py, px = self.direction[chain[-1][0], chain[-1][1], 1:3].astype(np.int32)
                chain.append((int(py), int(px)))
            for v, u in zip(chain[-2::-1], chain[:0:-1]):
                m = MOVES.index((v[0] - u[0], v[1] - u[1]))
                assert valid[m, u[0], u[1]]
                done[v] = np.float32(done[u] + weight[m, u[0], u[1]])
        return done


def path_cost32(free, cells, weights=None):
    """the binary32 sum of the move weights along `cells` [(y, x), ...], left to right; raises when a step is no free table move"""
    valid, weight = (weights if weights is not None else move_weights(free))[:2]
    g = np.float32(0)
    for (y, x), (vy, vx) in zip(cells[:-1], cells[1:]):
        m = MOVES.index((vy - y, vx - x))
        assert valid[m, y, x], ("blocked move", (y, x), (vy, vx))
        g = np.float32(g + weight[m, y, x])
    return g


# ---- the map families -----------------------------------------------------------------------------------------------------------

def _case(label, start, goals, free=None, points=None, cam_height=0.5, cell=0.05, center=(0.0, 0.0)):
    """label [H, W]: 0 unknown, 1 occupied, 2 free.  free defaults to label == 2 (the planner takes free_space as an input)."""
    label = np.asarray(label, np.int64)
    H, W = label.shape
    occ_map = np.zeros((3, H, W), np.float32)
    occ_map[0][label == 0] = 1
    occ_map[1][label == 1] = 1
    occ_map[2][label == 2] = 2
    free = (label == 2) if free is None else free
    return dict(H=H, W=W, occ_map=occ_map, free=np.ascontiguousarray(free, np.uint8), start=(int(start[0]), int(start[1])),
                goals=[(int(a), int(b)) for a, b in goals], points=points, cam_height=cam_height, cell=cell, center=center)


def _goals(label, start, extra=(), n=21, seed=0):
    """n goals: `extra`, then next to the start, on the borders, and drawn cells of every label"""
    H, W = label.shape
    rng = np.random.default_rng(seed)
    fixed = list(extra) + [(start[0], min(start[1] + 1, W - 1)), (min(start[0] + 2, H - 1), start[1]), (0, W // 2), (H - 1, W - 1), (H // 2, 0), (0, 0)]
    drawn = [(int(rng.integers(H)), int(rng.integers(W))) for _ in range(max(n - len(fixed), 0))]
    return (fixed + drawn)[:n]


def point_at(col, row, W, H, cell=0.05, center=(0.0, 0.0), y=0.2):
    """a Gaussian mean in the middle of cell (col, row) under fr_occ_cells_of's rule"""
    tx, tz = col - (W - 1) // 2 + 0.5, row - (H - 1) // 2 + 0.5
    return [center[0] + tx * cell, y, center[1] + tz * cell]


def serpentine(H, W, lane=12, gap=9, start=(2, 3), n_goals=21):
    """walls every `lane` rows, open for `gap` cells at alternating ends: the path runs the width of the map back and forth"""
    label = np.full((H, W), 2)
    for k, y in enumerate(range(lane - 4, H - 4, lane)):
        if k % 2:
            label[y, gap:] = 1
        else:
            label[y, :W - gap] = 1
    return _case(label, start, _goals(label, start, extra=[(H - 2, W // 2), (lane - 4, 0), (lane + 2, W - 3)], n=n_goals))


def make_case(family):
    H, W = 46, 52
    if family == "empty-room":
        label = np.full((H, W), 2)
        s = (H // 2, W // 2)
        return _case(label, s, _goals(label, s))
    if family.startswith("door-"):
        width = int(family.split("-")[1])
        label = np.full((H, W), 2)
        label[:, 25] = 1
        label[20:20 + width, 25] = 2
        s = (22, 8)
        return _case(label, s, _goals(label, s, extra=[(22, 40), (5, 45), (22, 25), (22, 26)]))
    if family == "serpentine":
        return serpentine(H, W)
    if family == "two-routes":
        # a slab with a corridor 5 cells wide through it: the straight way hugs walls, the way round runs clear
        label = np.full((100, 100), 2)
        label[20:80, 40:61] = 1
        label[20:80, 48:53] = 2
        s = (8, 50)
        return _case(label, s, _goals(label, s, extra=[(92, 50), (50, 50), (50, 20)], n=8))
    if family == "island":
        label = np.full((H, W), 2)
        label[10:30, 30] = label[10:30, 48] = 1
        label[10, 30:49] = label[29, 30:49] = 1
        s = (35, 10)
        return _case(label, s, _goals(label, s, extra=[(20, 40), (12, 32), (10, 30)]))
    if family == "start-outside-free":
        label = np.full((H, W), 2)
        label[10:14, 10:14] = 0
        s = (12, 12)
        return _case(label, s, _goals(label, s))
    if family in ("ring-7", "ring-8"):
        label = np.full((H, W), 2)
        y, x = 20, 20
        for cy, cx in [(y, x - 2), (y - 2, x), (y + 2, x)] + ([(y, x + 2)] if family == "ring-8" else []):
            label[cy, cx] = 1
        return _case(label, (y, x), _goals(label, (y, x)))
    if family == "start-corner":
        label = np.full((H, W), 2)
        label[15, 5:30] = 1
        return _case(label, (0, 0), _goals(label, (0, 0)))
    if family == "start-border":
        label = np.full((H, W), 2)
        label[15, 5:30] = 1
        return _case(label, (H - 1, 17), _goals(label, (H - 1, 17)))
    if family == "tier-thresholds":
        # one obstacle; the cells at L1 distance 5 | 6, 10 | 11, 20 | 21 from it lie on the start's row and on a diagonal
        label = np.full((50, 64), 2)
        label[25, 10] = 1
        s = (25, 40)
        return _case(label, s, _goals(label, s, extra=[(25, 15), (25, 16), (25, 20), (25, 21), (25, 30), (25, 31), (22, 12), (21, 12)]))
    if family == "gaussians":
        label = np.full((H, W), 2)
        cam = 1.5
        pts = []
        for col, row, n, ys in [(10, 10, 51, [1.0] * 49 + [cam, cam - 1.0]),               # 51 in the band, both ends of it included: occupied
                                (20, 10, 50, [1.0] * 50),                                  # 50: not
                                (30, 10, 51, [cam + 0.01] * 51),                           # above the band
                                (40, 10, 51, [cam - 1.01] * 51),                           # below it
                                (10, 30, 52, [1.0] * 26 + [2.0] * 26),                     # half of them in the band
                                (0, 45, 51, [1.0] * 51), (51, 0, 51, [1.0] * 51)]:         # border cells
            pts += [point_at(col, row, W, H, y=y) for y in ys[:n]]
        pts += [[1e3, 1.0, 0.0]] * 51 + [[-1.4, 1.0, 0.0]] * 51 + [[0.0, 1.0, 1.3]] * 51 + [[0.0, 1.0, -1.2]] * 51      # outside the grid
        s = (22, 25)
        return _case(label, s, _goals(label, s, extra=[(10, 10), (11, 11), (10, 20), (12, 12)]), points=np.array(pts, np.float32), cam_height=cam)
    raise ValueError(family)


FAMILIES = ("empty-room", "door-1", "door-3", "door-9", "serpentine", "two-routes", "island", "start-outside-free", "ring-7", "ring-8",
            "start-corner", "start-border", "tier-thresholds", "gaussians")


# ---- the g++ harness ----------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_plan_harness", harness_build.EXACT))
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    h.frp_h_grid.argtypes = [ci, ci, vp, vp, ci, cf, cf, cf, cf, ci, ci, vp, vp]
    h.frp_h_grid.restype = None
    h.frp_h_tiers.argtypes = [ci, ci, vp, vp]
    h.frp_h_tiers.restype = None
    h.frp_h_field.argtypes = [ci, ci, vp, ci, ci, vp]
    h.frp_h_field.restype = ci
    h.frp_h_paths.argtypes = [ci, ci, vp, vp, ci, ci, vp, ci, ci, vp, ci, vp]
    h.frp_h_paths.restype = None
    return h


def harness_grid(h, c, points="case"):
    H, W = c["H"], c["W"]
    pts = c["points"] if isinstance(points, str) else points
    pts = None if pts is None else np.ascontiguousarray(pts, np.float32)
    occ_map = np.ascontiguousarray(c["occ_map"], np.float32)
    occ_plan, status = np.zeros((H, W), np.uint8), np.zeros(STATUS_WORDS, np.int32)
    h.frp_h_grid(H, W, occ_map.ctypes.data, None if pts is None else pts.ctypes.data, 0 if pts is None else len(pts), c["cell"], c["center"][0],
                 c["center"][1], c["cam_height"], c["start"][0], c["start"][1], occ_plan.ctypes.data, status.ctypes.data)
    return occ_plan, status


def harness_tiers(h, free):
    free = np.ascontiguousarray(free, np.uint8)
    tiers = np.zeros_like(free)
    h.frp_h_tiers(free.shape[0], free.shape[1], free.ctypes.data, tiers.ctypes.data)
    return tiers


def harness_field(h, tiers, start):
    field = np.zeros(tiers.shape, np.uint64)
    in_free = h.frp_h_field(tiers.shape[0], tiers.shape[1], tiers.ctypes.data, start[0], start[1], field.ctypes.data)
    return field, int(in_free)


def harness_paths(h, field, occ_plan, start, goals, shortcut, max_len=None):
    """(paths int32 [G, max_len, 2], lengths int32 [G])"""
    H, W = occ_plan.shape
    G = len(goals)
    max_len = H * W + 1 if max_len is None else max_len
    g = np.ascontiguousarray(np.asarray(goals, np.int32).reshape(G, 2))
    paths, lengths = np.zeros((G, max_len, 2), np.int32), np.zeros(G, np.int32)
    field, occ_plan = np.ascontiguousarray(field, np.uint64), np.ascontiguousarray(occ_plan, np.uint8)
    h.frp_h_paths(H, W, field.ctypes.data, occ_plan.ctypes.data, start[0], start[1], g.ctypes.data, G, int(shortcut), paths.ctypes.data, max_len,
                  lengths.ctypes.data)
    return paths, lengths


def harness_plan(h, c, shortcut=True, points="case"):
    """everything the harness computes for a case: dict(occ_plan, status, tiers, field, in_free, paths [list of (M, 2)], lengths)"""
    occ_plan, status = harness_grid(h, c, points)
    tiers = harness_tiers(h, c["free"])
    field, in_free = harness_field(h, tiers, c["start"])
    paths, lengths = harness_paths(h, field, occ_plan, c["start"], c["goals"], shortcut)
    return dict(occ_plan=occ_plan, status=status, tiers=tiers, field=field, in_free=in_free, lengths=lengths,
                paths=[paths[g, :max(int(n), 0)].astype(np.int64) for g, n in enumerate(lengths)])
