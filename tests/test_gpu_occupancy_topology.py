"""Planner-side kernels (csrc/fisher_occ.hip, planning/astar.py) on adversarial maps and edge shapes, against the CPU restatement
of the reference planner (oracle/occupancy_frontier.py).  tests/test_gpu_occupancy.py only ever sees maps grown from depth views
of one convex room; here the maps are synthetic label images (tests/occ_patterns.py, whose properties
tests/test_occ_patterns_cpu.py checks without a GPU): long chains, corner-only contacts, many components in one wave, exact
ties, the size > min_area boundary, a map taller than the row scan's 1024 threads, ragged images, bad depth, a map smaller than
the room, the camera on the map's border, the thresholds of the free-space step, and one workspace shared by every entry point.
Every comparison is exact.  `combined` and `closest` pick by means of fp64 atomic sums, whose order is free: each such
comparison first requires, on the CPU, that the restatement's best and second-best key differ by more than 1e-9 relative
(reordering at most 1e5 fp64 terms moves a sum by about 1e-11)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import occ_patterns as op

pytestmark = pytest.mark.gpu

METHODS = ("combined", "largest", "closest")
_CODE = {"largest": 0, "combined": 1, "closest": 2}
SENTINEL = -7


def _K(W, H):
    """square pixels, 90 degrees across the width (also for the one-row image)"""
    return np.array([[W / 2.0, 0.0, W / 2.0], [0.0, W / 2.0, H / 2.0], [0.0, 0.0, 1.0]], dtype=np.float32)


def _planner(gpu, occ, cam, method="combined", K=None):
    """An AstarPlanner holding the (3, gh, gw) map `occ` in a fresh tensor, centred on the origin, camera cell (row, col) = cam."""
    from planning import AstarPlanner
    pl = AstarPlanner(device=gpu, cell_size=0.05, frontier_select_method=method)
    _, gh, gw = occ.shape
    pl.grid_dim = np.array([gw, gh])
    pl._map_center_np = np.zeros(2, dtype=np.float32)
    pl.map_center = torch.zeros(2, device=gpu)
    pl.occ_map = torch.from_numpy(np.ascontiguousarray(occ, dtype=np.float32)).to(gpu)
    pl.cam_pos = np.array([int(cam[0]), int(cam[1])])
    pl.intrinsics = K
    pl.cam_height = 0.0
    return pl


def _pair(gpu, label, cam, method="combined", K=None):
    pl = _planner(gpu, op.onehot(label), cam, method, K)
    om = op.oracle_map(label, cam, intrinsics=K, height_range=(pl.height_lower, pl.height_upper), far=pl.pcd_far_distance)
    return pl, om


def _frontiers_direct(pl, free, method, max_cells=None):
    """fr_occ_frontiers through the C ABI: (frontier, target, cells, counts); `cells` is the whole sentinel-filled buffer."""
    from fisher_rast import _lib
    lib = _lib.load()
    dev = pl.occ_map.device
    cfg = pl._occ_cfg()
    ws, need = pl._occ_workspace(cfg)
    gh, gw = int(pl.grid_dim[1]), int(pl.grid_dim[0])
    free_dev = torch.from_numpy(np.ascontiguousarray(free, dtype=np.uint8)).to(dev)
    frontier = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    target = torch.empty((gh, gw), dtype=torch.uint8, device=dev)
    cells = torch.full((gh * gw, 2), SENTINEL, dtype=torch.int32, device=dev)
    counts = torch.zeros((4,), dtype=torch.int32, device=dev)
    _lib.check(lib.fr_occ_frontiers(ctypes.byref(cfg), pl.occ_map.data_ptr(), free_dev.data_ptr(), int(pl.cam_pos[0]), int(pl.cam_pos[1]),
                                    _CODE[method], 10, frontier.data_ptr(), target.data_ptr(), cells.data_ptr(),
                                    gh * gw if max_cells is None else int(max_cells), counts.data_ptr(), ws.data_ptr(), need,
                                    pl._stream()), "fr_occ_frontiers")
    return frontier.cpu().numpy(), target.cpu().numpy(), cells.cpu().numpy(), counts.cpu().numpy()


def _require_key_gap(om, det, method):
    """The condition of the module docstring, asserted on the restatement alone."""
    if method == "largest" or det["frontier"].sum() == 0:
        return
    _, cc, sizes, qual = op.frontier_components(om.occ_map.argmax(axis=0), det["free"])
    gap = op.key_gap(op.selection_keys(cc, sizes, qual, om.cam_pos, method))
    assert gap > 1e-9, f"{method}: best and second-best key {gap} apart: not decidable from sums of free order"


def _check_frontiers(pl, om, method, points=None):
    """build_connected_freespace, build_frontiers and the raw fr_occ_frontiers outputs against the restatement."""
    pts_np = None if points is None else points.cpu().numpy()
    want_free = om.build_connected_freespace(pts_np)
    got_free = pl.build_connected_freespace(points)
    assert got_free.dtype == np.uint8 and np.array_equal(got_free, want_free), f"{(got_free != want_free).sum()} free cells differ"
    det = {"free": want_free}
    want_pts, want_free2 = om.build_frontiers(pts_np, method=method, details=det)
    _require_key_gap(om, det, method)
    pl.frontier_select_method = method
    # an out-of-range point (above the height window) makes build_frontiers return the whole cell list instead of the FBE pick
    probe = torch.tensor([[0.0, 50.0, 0.0]], device=pl.occ_map.device) if points is None else points
    got_pts, got_free2 = pl.build_frontiers(probe)
    assert np.array_equal(got_free2, want_free2)
    assert np.array_equal(pl.frontier, det["frontier"])
    assert (got_pts is None) == (want_pts is None)
    if want_pts is not None:
        assert np.array_equal(pl.target_frontier, det["target"])
        assert got_pts.shape == want_pts.shape and np.array_equal(got_pts, want_pts)
        if points is None:
            one, _ = pl.build_frontiers(None)                          # FBE rule (astar.py:655-679) on the same cells
            d = np.linalg.norm(want_pts - om.cam_pos[None, :], axis=1)
            ok = np.where(d >= 0.5)[0]
            assert one.shape == (1, 2) and np.array_equal(one[0], want_pts[ok[np.argmin(d[ok])]])
    frontier, target, cells, counts = _frontiers_direct(pl, want_free2, method)
    want_target = det.get("target", np.zeros_like(want_free2))
    assert np.array_equal(frontier, det["frontier"]) and counts[0] == det["frontier"].sum()
    assert counts[1] == det.get("components", 0)
    assert np.array_equal(target, want_target) and counts[2] == want_target.sum()
    rows, cols = np.where(want_target)
    assert np.array_equal(cells[:counts[2]], np.stack([cols, rows], axis=1))
    assert (cells[counts[2]:] == SENTINEL).all()
    return det, (got_free, frontier, target, cells, counts)


# ---- 2. free space and frontiers on the patterns ----------------------------------------------------------------------------
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("name", sorted(op.cases()))
def test_patterns_match_the_restatement(gpu, name, method):
    label, cam = op.cases()[name]
    pl, om = _pair(gpu, label, cam, method)
    det, _ = _check_frontiers(pl, om, method)
    # what the pattern is for (tests/test_occ_patterns_cpu.py derives these numbers without the restatement)
    free = det["free"]
    if name.startswith("serpentine"):
        assert free.sum() == 36861
    elif name.startswith("diagonal"):
        assert free.sum() == 360
    elif name.startswith("rectangles"):
        assert free.sum() == 84 and np.where(free)[0].min() == 5
    elif name == "gapped_room" and method == "largest":
        assert det["components"] == 3 and det["target"].sum() == 24 and np.where(det["target"])[0].max() == 88
    elif name.startswith("perforated"):
        assert det["components"] > 100
    elif name.startswith("strip") and name.endswith("3"):
        assert det["frontier"].sum() == 3 and det["components"] == 0 and "target" not in det
    elif name.startswith("strip"):
        assert det["components"] == 1 and det["target"].sum() == 12


@pytest.mark.parametrize("name", ["serpentine", "spiral", "perforated"])
def test_repeated_runs_give_identical_bytes(gpu, name):
    """The union-find merges race; the result must not depend on who wins."""
    label, cam = op.cases()[name]
    pl, om = _pair(gpu, label, cam, "combined")
    runs = [_check_frontiers(pl, om, "combined")[1] for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert a.tobytes() == b.tobytes()


@pytest.mark.parametrize("method", METHODS)
def test_cell_list_truncates_at_max_cells(gpu, method):
    label, cam = op.cases()["perforated"]
    pl, om = _pair(gpu, label, cam, method)
    det = {}
    _, free = om.build_frontiers(None, method=method, details=det)
    rows, cols = np.where(det["target"])
    n = len(rows)
    assert n >= 25
    for cap in (0, 7, n - 1, n, n + 5):
        frontier, target, cells, counts = _frontiers_direct(pl, free, method, max_cells=cap)
        k = min(cap, n)
        assert counts[2] == n and np.array_equal(target, det["target"])
        assert np.array_equal(cells[:k], np.stack([cols, rows], axis=1)[:k])
        assert (cells[k:] == SENTINEL).all()


# ---- 3. a map taller than the row scan's 1024 threads ---------------------------------------------------------------------
def _tall_label():
    """70 x 2051: a free hall behind occupied side walls on an unknown background; the walls are unknown along 12 cells in the
    rows below 1024 and between 1024 and 2048, and the hall's short ends are open (unknown): two frontier components of equal
    size, the later one in rows 2048..2050."""
    gh, gw = 2051, 70
    lab = np.full((gh, gw), op.UNKNOWN, dtype=np.uint8)
    lab[4:2049, 9:61] = op.OCCUPIED
    lab[4:2049, 10:60] = op.FREE
    lab[500:512, 9] = op.UNKNOWN
    lab[1500:1512, 60] = op.UNKNOWN
    return lab


@pytest.mark.parametrize("method,cam", [("largest", (1000, 30)), ("closest", (506, 20)), ("closest", (1490, 50)), ("closest", (2045, 25)),
                                        ("combined", (1200, 33))])
def test_tall_map_row_scan(gpu, method, cam):
    from scipy import ndimage
    from oracle.occupancy_frontier import free_candidates
    label = _tall_label()
    pl, om = _pair(gpu, label, cam, method)
    det, _ = _check_frontiers(pl, om, method)
    trows = np.where(det["target"])[0]
    if method == "largest":                                            # the open ends: the bottom one wins the tie, rows above 2048
        assert trows.min() == 2048 and trows.max() == 2050 and len(trows) == 162
    elif method == "closest":
        assert abs(int(np.median(trows)) - cam[0]) < 20
    free = det["free"]
    assert free[:1024].any() and free[1024:2048].any() and free[2048:].any()
    er11 = ndimage.binary_erosion(free.astype(bool), structure=np.ones((11, 11), bool), border_value=1).astype(np.uint8)
    rp = pl.sample_random_candidate(np.array([0.0, 0.4, 0.0]), free, seed=41)
    want = free_candidates(er11, 0.4, 41, grid_dim=(70, 2051))
    assert rp.shape == want.shape and rp.shape[0] == int(er11.sum()) // 4 > 1000
    assert np.array_equal(rp[:, :3, 3].cpu().numpy(), want[:, :3, 3])       # the cells the draws picked, rows in all three thirds
    z = want[:, 2, 3] / 0.05 + 1025
    assert (z < 1024).any() and ((z > 1024) & (z < 2048)).any()


# ---- 4. thresholds of the free-space step ----------------------------------------------------------------------------------
def _points_in_cell(col, row, n, gw, gh, y=0.0):
    """n points in the middle of cell (col, row) of a map centred on the origin (datasets/util/map_utils.py:106-125)."""
    x = (col - (gw - 1) // 2 + 0.5) * 0.05
    z = (row - (gh - 1) // 2 + 0.5) * 0.05
    return np.tile(np.array([[x, y, z]], dtype=np.float32), (n, 1))


def _check_cells(pts, gw, gh, want):
    from oracle.occupancy_frontier import discretize_coords
    got = discretize_coords(pts[:, 0], pts[:, 2], (gw, gh), 0.05, (0.0, 0.0))
    assert np.array_equal(got, np.asarray(want))


def test_point_count_height_and_clamp_thresholds(gpu):
    gw, gh = 41, 30
    label = np.full((gh, gw), op.FREE, dtype=np.uint8)
    lo, hi = np.float32(-0.6), np.float32(0.6)
    below, above = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    assert below < lo and above > hi
    groups = [
        (_points_in_cell(5, 5, 25, gw, gh), (5, 5), False),             # exactly 25: stays
        (_points_in_cell(9, 5, 26, gw, gh), (9, 5), True),              # 26: blocked
        (np.concatenate([_points_in_cell(5, 12, 13, gw, gh, lo), _points_in_cell(5, 12, 13, gw, gh, hi)]), (5, 12), True),   # on the bounds: kept
        (np.concatenate([_points_in_cell(9, 12, 25, gw, gh, lo), _points_in_cell(9, 12, 1, gw, gh, below),
                         _points_in_cell(9, 12, 1, gw, gh, above)]), (9, 12), False),       # one ulp outside: dropped, 25 left
    ]
    far = 400.0                                                        # far outside on all four sides: clamps into border cells
    for (x, z), cell in ((( -far, (20 - 14 + 0.5) * 0.05), (0, 20)), ((far, (8 - 14 + 0.5) * 0.05), (gw - 1, 8)),
                         (((3 - 20 + 0.5) * 0.05, -far), (3, 0)), (((15 - 20 + 0.5) * 0.05, far), (15, gh - 1)),
                         ((-far, -far), (0, 0)), ((far, far), (gw - 1, gh - 1))):
        groups.append((np.tile(np.array([[x, 0.0, z]], dtype=np.float32), (26, 1)), cell, True))
    for pts, cell, _ in groups:
        _check_cells(pts, gw, gh, [cell] * len(pts))
    pts = np.concatenate([g[0] for g in groups])
    rng = np.random.default_rng(5)
    pts = pts[rng.permutation(len(pts))]
    cam = (14, 7)
    pl, om = _pair(gpu, label, cam)
    # the restatement's blocked set is the planted one
    inr = pts[(pts[:, 1] >= lo) & (pts[:, 1] <= hi)]
    from oracle.occupancy_frontier import discretize_coords
    uv, cnt = np.unique(discretize_coords(inr[:, 0], inr[:, 2], (gw, gh), 0.05, (0.0, 0.0)), axis=0, return_counts=True)
    assert sorted(map(tuple, uv[cnt > 25])) == sorted(c for _, c, blocked in groups if blocked)
    assert sorted(map(tuple, uv[cnt == 25])) == sorted(c for _, c, blocked in groups if not blocked)
    for method in METHODS:
        _check_frontiers(pl, om, method, torch.from_numpy(pts).to(gpu))
    free = om.build_connected_freespace(pts)
    assert free[5, 5] and free[12, 9] and not free[5, 9] and not free[12, 5] and not free[0, 0] and not free[20, 0]
    assert not np.array_equal(free, om.build_connected_freespace(None))


@pytest.mark.parametrize("n_free", [18, 19])
def test_free_cell_count_threshold(gpu, n_free):
    """The points only block when the map has MORE than 18 free cells before the opening (astar.py:419)."""
    gw, gh = 23, 17
    label = np.full((gh, gw), op.OCCUPIED, dtype=np.uint8)
    label[6:9, 4:10] = op.FREE                                         # 3 x 6 = 18
    if n_free == 19:
        label[12, 15] = op.FREE                                        # a lone cell: counted, then removed by the opening
    assert (label == op.FREE).sum() == n_free
    pts = _points_in_cell(9, 7, 26, gw, gh)
    _check_cells(pts, gw, gh, [(9, 7)] * 26)
    pl, om = _pair(gpu, label, (7, 6))
    _check_frontiers(pl, om, "combined", torch.from_numpy(pts).to(gpu))
    free = om.build_connected_freespace(pts)
    assert free.sum() == (18 if n_free == 18 else 15)


def test_argmax_ties_take_the_first_layer(gpu):
    gw, gh = 45, 33
    occ = np.zeros((3, gh, gw), dtype=np.float32)
    occ[2] = 1.0                                                       # free everywhere ...
    ties = {(1, 1, 1): 0, (0, 1, 1): 1, (1, 0, 1): 0, (0, 0, 0): 0}     # ... but for four 4 x 4 patches: layers -> expected label
    for k, v in enumerate(ties):
        occ[:, 8:12, 5 + 10 * k:9 + 10 * k] = np.asarray(v, dtype=np.float32)[:, None, None]
    label = occ.argmax(axis=0)
    for k, (v, want) in enumerate(ties.items()):
        assert (label[8:12, 5 + 10 * k:9 + 10 * k] == want).all()
    cam = (20, 13)
    pl = _planner(gpu, occ, cam)
    om = op.oracle_map(label, cam)
    om.occ_map = occ.copy()
    for method in METHODS:
        det, _ = _check_frontiers(pl, om, method)
    assert det["free"].sum() == gw * gh - 4 * 16 and det["frontier"].sum() == 3 * 12     # the occupied patch has no frontier


# ---- 5. update edges: occ_map bit-exact after every frame ------------------------------------------------------------------
def _update_pair(gpu, gw, gh, W, H, unknown=1.0):
    """All cells unknown, as after init.  One frame adds about 1 to a cell's free or occupied layer, which only ties with init's
    1.0 (and the first maximum is `unknown`); a weaker prior lets a single frame decide."""
    K = _K(W, H)
    label = np.zeros((gh, gw), dtype=np.uint8)
    pl, om = _pair(gpu, label, (gh // 2, gw // 2), K=K)
    if unknown != 1.0:
        pl.occ_map.mul_(unknown)
        om.occ_map *= np.float32(unknown)
        assert np.array_equal(pl.occ_map.cpu().numpy(), om.occ_map)
    return pl, om, K


def _poses(n, seed, scale=1.0):
    from fisher_rast import synthetic
    p = synthetic.candidate_poses(n, seed).numpy().astype(np.float32)
    p[:, [0, 2], 3] *= np.float32(scale)
    return p


def _step(pl, om, depth, pose, t, downsample=1):
    pl.update_occ_map(depth, torch.from_numpy(pose).to(pl.occ_map.device), t, downsample=downsample)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)                # inf * 0 and NaN comparisons in the planted depth
        with np.errstate(all="ignore"):
            om.update_occ_map(depth, pose, downsample=downsample)
    got = pl.occ_map.cpu().numpy()
    assert np.array_equal(pl.cam_pos, om.cam_pos)
    assert np.array_equal(got, om.occ_map), f"frame {t}: {(got != om.occ_map).sum()} cells differ, max {np.nanmax(np.abs(got - om.occ_map))}"


@pytest.mark.parametrize("W,H,downsample", [(50, 37, 1), (97, 61, 3), (65, 1, 1), (7, 5, 2)])
def test_update_with_ragged_images(gpu, W, H, downsample):
    """Pixel counts that are no multiple of the wave, strides that do not divide the image."""
    from oracle.occupancy_frontier import room_depth
    pl, om, K = _update_pair(gpu, 257, 193, W, H)
    nx, ny = -(-W // downsample), -(-H // downsample)
    assert (nx * ny) % 64 != 0
    for t, p in enumerate(_poses(4, 310 + W)):
        _step(pl, om, room_depth(p, W, H, K), p, t, downsample)
    assert (om.occ_map[2] > 0).sum() > 50 and (om.occ_map[1] > 0).sum() > 0           # free and occupied evidence was written


def test_update_with_bad_depth(gpu):
    """Zero, negative, NaN, +inf, exactly far_distance and the float32 just below it."""
    from oracle.occupancy_frontier import room_depth
    W, H = 50, 37
    pl, om, K = _update_pair(gpu, 257, 193, W, H)
    far = np.float32(pl.pcd_far_distance)
    rng = np.random.default_rng(11)
    for t, p in enumerate(_poses(3, 320)):
        d = room_depth(p, W, H, K).copy()
        flat = d.reshape(-1)
        where = rng.permutation(flat.size)[:600].reshape(6, 100)
        for w, v in zip(where, (0.0, -1.5, np.nan, np.inf, far, np.nextafter(far, np.float32(0)))):
            flat[w] = v
        flat[W * (H // 2) + W // 2] = np.inf                            # the principal ray: x = y = 0 times inf
        _step(pl, om, d, p, t)
    assert np.isfinite(om.occ_map).all()


def test_update_on_a_map_smaller_than_the_room(gpu):
    """96 x 80 cells of 0.05 m inside the 10 m room: most depth points clamp into border cells and the free lines start there.
    The last camera stands outside the map."""
    from oracle.occupancy_frontier import room_depth
    W, H = 50, 37
    pl, om, K = _update_pair(gpu, 96, 80, W, H)
    poses = _poses(5, 330, scale=0.3)
    poses[-1, [0, 2], 3] = [3.13, -2.72]
    for t, p in enumerate(poses):
        _step(pl, om, room_depth(p, W, H, K), p, t)
        if t < 4:
            assert 0 <= pl.cam_pos[0] < 80 and 0 <= pl.cam_pos[1] < 96
    assert pl.cam_pos[0] < 0 and pl.cam_pos[1] >= 96
    seen_occupied = om.occ_map[1] > 0
    border = np.ones_like(seen_occupied)
    border[1:-1, 1:-1] = False
    assert seen_occupied[border].sum() > 20 and seen_occupied[~border].sum() == 0


@pytest.mark.parametrize("row,col", [(0, 40), (33, 0), (79, 51), (41, 95), (0, 0), (79, 95), (0, 95), (79, 0)])
def test_update_with_the_camera_on_the_border(gpu, row, col):
    """occ_map[2, z-1:z+2, x-1:x+2] = 1e3 is a slice (astar.py:214): clipped past the last row / column, EMPTY in row 0 and column 0,
    where it starts at -1."""
    from oracle.occupancy_frontier import room_depth
    W, H = 50, 37
    gw, gh = 96, 80
    pl, om, K = _update_pair(gpu, gw, gh, W, H)
    before = om.occ_map.copy()
    for t, p in enumerate(_poses(2, 340 + row + col)):
        p[0, 3] = np.float32((col + 0.5 - gw // 2) * 0.05)
        p[2, 3] = np.float32((row + 0.5 - gh // 2) * 0.05)
        _step(pl, om, room_depth(p, W, H, K), p, t)
        assert tuple(pl.cam_pos) == (row, col)
    marked = (om.occ_map[2] - before[2]) > 500.0
    want = np.zeros_like(marked)
    if row > 0 and col > 0:
        want[row - 1:row + 2, col - 1:col + 2] = True
    assert np.array_equal(marked, want)


# ---- 6. one workspace behind every entry point ---------------------------------------------------------------------------------
class _Sequence:
    """update, build_frontiers(points), sample_random_candidate, generate_candidate_in_freespace, update,
    build_connected_freespace(points), update, build_frontiers(None) on one planner, the restatement alongside."""

    def __init__(self, gpu, gw, gh, seed):
        from fisher_rast import synthetic
        self.W, self.H = 50, 37
        self.gw, self.gh = gw, gh
        self.pl, self.om, self.K = _update_pair(gpu, gw, gh, self.W, self.H, unknown=0.5)
        self.poses = _poses(3, seed, scale=0.25)
        self.points = synthetic.room_shell(20_000, seed)["means3D"].to(gpu)
        self.t = 0
        self.gpu = gpu
        self.steps = [self.update, self.frontiers_points, self.random_candidates, self.ring_candidates, self.update, self.freespace_points,
                      self.update, self.frontiers_none]

    def update(self):
        from oracle.occupancy_frontier import room_depth
        p = self.poses[self.t]
        _step(self.pl, self.om, room_depth(p, self.W, self.H, self.K), p, self.t)
        self.t += 1

    def frontiers_points(self):
        self.free = _check_frontiers(self.pl, self.om, "combined", self.points)[0]["free"]
        assert self.free.sum() > 100

    def frontiers_none(self):
        for method in METHODS:
            _check_frontiers(self.pl, self.om, method)

    def freespace_points(self):
        want = self.om.build_connected_freespace(self.points.cpu().numpy())
        assert np.array_equal(self.pl.build_connected_freespace(self.points), want)

    def random_candidates(self):
        from scipy import ndimage
        from oracle.occupancy_frontier import free_candidates
        er = ndimage.binary_erosion(self.free.astype(bool), structure=np.ones((11, 11), bool), border_value=1).astype(np.uint8)
        rp = self.pl.sample_random_candidate(np.array([0.0, 0.3, 0.0]), self.free, seed=17)
        want = free_candidates(er, 0.3, 17, grid_dim=(self.gw, self.gh))
        assert rp.shape == want.shape and rp.shape[0] > 4 and np.array_equal(rp[:, :3, 3].cpu().numpy(), want[:, :3, 3])

    def ring_candidates(self):
        """the fused filter against the restatement's rule on the kernel's own positions (as tests/test_gpu_occupancy.py does)"""
        from scipy import ndimage
        pl = self.pl
        centers = torch.from_numpy(self.poses[:, [0, 2], 3]).to(self.gpu)
        pl.K = 200
        cand = pl.generate_candidate(centers, seed=23)
        kept = pl.generate_candidate_in_freespace(centers, self.free, seed=23)
        er = ndimage.binary_erosion(self.free.astype(bool), structure=np.ones((10, 10), bool), border_value=1)
        xy = cand[:, [0, 2], 3].cpu().numpy()
        col = (xy[:, 0] / np.float32(0.05) + np.float32(self.gw // 2)).astype(np.int64)
        row = (xy[:, 1] / np.float32(0.05) + np.float32(self.gh // 2)).astype(np.int64)
        inside = (col >= 0) & (col < self.gw) & (row >= 0) & (row < self.gh)
        keep = np.zeros(len(col), dtype=bool)
        keep[inside] = er[row[inside], col[inside]]
        assert er.sum() > 40 and 0 < keep.sum() < len(keep)
        assert torch.equal(kept, cand[torch.from_numpy(keep).to(self.gpu)])


def test_workspace_reuse_sequence(gpu):
    seq = _Sequence(gpu, 130, 97, 350)
    for step in seq.steps:
        step()


def test_two_planners_take_turns(gpu):
    a, b = _Sequence(gpu, 130, 97, 351), _Sequence(gpu, 96, 80, 352)
    for sa, sb in zip(a.steps, b.steps):
        sa()
        sb()
