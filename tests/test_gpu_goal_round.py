"""-m gpu: the object round on the device (fr_plan_actions_object, csrc/fr_action_object.hip; fr_occ_object_cells and
fr_occ_grid_candidates, csrc/fr_goal.hip) and the Python layer on it (planning/astar.py: GoalSelectOps, PathPlanOps.plan_actions_object;
fisher_rast/plan_round.py: plan_best_object_path).

Through the C ABI on guarded buffers: the follower over every case family of tests/goal_cases.py against the g++ harness over the same
headers, bit for bit -- actions, counts, keep flags, cells, pruned paths equal, the binary32 inverses and the positions equal as bits --
and against the NumPy restatement of the reference loop by the CPU test's bars; zeros behind every list; guards intact; once on a
non-default stream.  The object cells against np.unique; the sorted grid against a float32 NumPy restatement on the same draws
(2e-6, at most one boundary keep flag).  Through the Python layer on a 96 x 96 two-room map."""
import ctypes
import types

import numpy as np
import pytest
import torch

import goal_cases as gc

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes behind every buffer
GUARD_BYTE = 0x5A
Q = gc.Q


@pytest.fixture(scope="module")
def harness():
    return gc.build_harness()


class _Guarded:
    """a device buffer of n bytes (256-byte aligned), filled with the guard pattern, with GUARD more bytes behind it"""

    def __init__(self, n, dev):
        self.buf = torch.full((n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.n = n

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, dtype):
        return self.buf[:self.n].cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.buf[self.n:] == GUARD_BYTE).all())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _cfg(W, H, cell, center):
    from fisher_rast import _lib
    return _lib.OccCfg(W, H, cell, center[0], center[1], -0.6, 0.6, 10.0)


def _f64x16(m):
    return (ctypes.c_double * 16)(*[float(v) for v in np.asarray(m, np.float64).reshape(-1)])


# ---- fr_plan_actions_object ------------------------------------------------------------------------------------------------------------

def _device_plan(dev, c, staged=None):
    """fr_plan_actions_object on guarded buffers on the current stream: the layout of gc.harness_plan, and `intact`"""
    from fisher_rast import _lib
    lib = _lib.load()
    a = gc.case_arrays(c)
    G, L = len(a["lengths"]), c["max_len"] + 1
    d = staged if staged is not None else {k: torch.from_numpy(a[k]).to(dev) for k in ("paths", "lengths", "goals", "goals_c2w")}
    b = dict(actions=_Guarded(G * Q, dev), n=_Guarded(4 * G, dev), keep=_Guarded(G, dev), w2c=_Guarded(64 * G * Q, dev), xz=_Guarded(16 * G * Q, dev),
             cells=_Guarded(8 * G * Q, dev), pruned=_Guarded(8 * G * L, dev), plen=_Guarded(4 * G, dev))
    cfg = _cfg(c["W"], c["H"], c["cell"], c["center"])
    _lib.check(lib.fr_plan_actions_object(ctypes.byref(cfg), d["paths"].data_ptr(), c["max_len"], d["lengths"].data_ptr(), d["goals"].data_ptr(),
                                          d["goals_c2w"].data_ptr(), G, _f64x16(c["agent"]), c["cam_height"], c["step"], c["turn"], c["cell"],
                                          b["actions"].ptr, b["n"].ptr, b["keep"].ptr, b["w2c"].ptr, b["xz"].ptr, b["cells"].ptr, b["pruned"].ptr,
                                          b["plen"].ptr, _stream(dev)), "fr_plan_actions_object")
    torch.cuda.current_stream(dev).synchronize()
    return dict(actions=b["actions"].get(np.uint8).reshape(G, Q), n_actions=b["n"].get(np.int32), keep=b["keep"].get(np.uint8),
                w2c=b["w2c"].get(np.float32).reshape(G, Q, 4, 4), c2w_xz=b["xz"].get(np.float64).reshape(G, Q, 2),
                map_xz=b["cells"].get(np.int32).reshape(G, Q, 2), pruned=b["pruned"].get(np.int32).reshape(G, L, 2),
                pruned_len=b["plen"].get(np.int32), intact=all(g.intact() for g in b.values()))


_WANT = {}


def _expected(h, family):
    """the case, the harness's answer and the restatement's -- once per family, shared by the tests, never written to"""
    if family not in _WANT:
        c = gc.make_case(family)
        _WANT[family] = (c, gc.harness_plan(h, c), gc.np_action_planning_object_adv(c))
    return _WANT[family]


def _check(c, got, hw, want):
    assert got["intact"], "a guard behind an output was written"
    # the harness over the same headers: bit for bit
    for k in ("actions", "n_actions", "keep", "map_xz", "pruned", "pruned_len"):
        assert np.array_equal(got[k], hw[k]), (c["name"], k)
    assert np.array_equal(got["w2c"].view(np.uint32), hw["w2c"].view(np.uint32)), c["name"]
    assert np.array_equal(got["c2w_xz"].view(np.uint64), hw["c2w_xz"].view(np.uint64)), c["name"]
    # and the restatement of the reference loop: the margins first, then the CPU test's bars; zeros behind every list
    gc.compare(got, want, c)


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_follower_equals_harness_bit_for_bit_and_the_restatement(gpu, harness, family):
    c, hw, want = _expected(harness, family)
    _check(c, _device_plan(gpu, c), hw, want)


def test_follower_on_a_side_stream_in_stream_order(gpu, harness):
    c, hw, want = _expected(harness, "g70")
    a = gc.case_arrays(c)
    host = {k: torch.from_numpy(a[k]).pin_memory() for k in ("paths", "lengths", "goals", "goals_c2w")}
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        # the inputs arrive on the side stream, behind a device-side detour: the kernels can only be right if they wait for them
        staged = {k: (v.to(gpu, non_blocking=True).clone().flip(0).flip(0)).contiguous() for k, v in host.items()}
        got = _device_plan(gpu, c, staged)
    _check(c, got, hw, want)


def test_empty_call_returns_without_a_launch(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    cfg = _cfg(96, 96, 0.05, (0.0, 0.0))
    out = _Guarded(4096, gpu)
    torch.cuda.synchronize()
    none = [None] * 8
    assert lib.fr_plan_actions_object(ctypes.byref(cfg), None, 4, None, None, None, 0, _f64x16(np.eye(4)), 0.4, 0.065, 10., 0.05, *none, _stream(gpu)) == _lib.FR_OK
    assert lib.fr_occ_grid_candidates(ctypes.byref(cfg), None, 0, None, None, 0, 0.2, 1.0, 24, 6, 0, 0.4, 1, None, 40, None, None, _stream(gpu)) == _lib.FR_OK
    torch.cuda.synchronize()
    assert bool((out.buf == GUARD_BYTE).all())


# ---- fr_occ_object_cells ---------------------------------------------------------------------------------------------------------------

def _cloud(rng, W, H, cell, center, n):
    """n points in a dozen clusters inside the map; from 300 on also cells with exactly 3 and exactly 4 points (in the map and, through
    points far outside it, in the border cells), and two rows that are not finite"""
    pts = np.zeros((n, 3), np.float32)
    if n:
        spots = rng.uniform(-0.9, 0.9, (12, 2)) * np.array([W, H]) * cell / 2 + np.asarray(center)
        pts[:, [0, 2]] = spots[rng.integers(0, 12, n)] + rng.uniform(-0.04, 0.04, (n, 2))
        pts[:, 1] = rng.uniform(-1, 1, n)
    if n >= 300:
        # cells of their own, on the discretisation's grid (its cell k spans k - (dim - 1) // 2 .. + 1, in cells, from the centre)
        for k, (col, row, m) in enumerate(((1, 1, 3), (2, 1, 4))):                # in the outer 3 %: no cluster reaches them
            x = (col - (W - 1) // 2 + 0.5) * cell + center[0]
            z = (row - (H - 1) // 2 + 0.5) * cell + center[1]
            pts[10 * k:10 * k + m, [0, 2]] = [x, z]
            pts[10 * k + m:10 * k + 10, [0, 2]] = spots[0]
        pts[20:23, [0, 2]] = [50.0, 50.0]                         # outside: 3 in the border cell (W - 1, H - 1)
        pts[23:27, [0, 2]] = [-50.0, 1e30]                        # 4 in (0, H - 1)
        pts[27] = [np.nan, 0, 0]
        pts[28] = [0, 0, np.inf]
    return pts


@pytest.mark.parametrize("grid", [(67, 71, 0.05, (0.37, -1.21)), (128, 128, 0.05, (0.0, 0.0))])
def test_object_cells_equal_np_unique(gpu, grid):
    from fisher_rast import _lib
    lib = _lib.load()
    W, H, cell, center = grid
    cfg = _cfg(W, H, cell, center)
    need = lib.fr_occ_workspace_bytes(ctypes.byref(cfg))
    rng = np.random.default_rng(7)
    for n in (0, 1, 300, 70000):
        pts = _cloud(rng, W, H, cell, center, n)
        d_pts = torch.from_numpy(pts).to(gpu)
        full_cells, full_counts = gc.np_object_cells(W, H, cell, center, pts, 3, W * H)
        if n >= 300:
            assert full_counts[1] == n - 2 and full_counts[0] > 4
            assert [2, 1] in full_cells.tolist() and [1, 1] not in full_cells.tolist()
            assert [0, H - 1] in full_cells.tolist() and [W - 1, H - 1] not in full_cells.tolist()
        for max_cells in (W * H, 2, 0):
            ws, cells, counts = _Guarded(need, gpu), _Guarded(8 * max_cells, gpu), _Guarded(8, gpu)
            _lib.check(lib.fr_occ_object_cells(ctypes.byref(cfg), d_pts.data_ptr() if n else None, n, 3, cells.ptr if max_cells else None, max_cells,
                                               counts.ptr, ws.ptr, need, _stream(gpu)), "fr_occ_object_cells")
            torch.cuda.synchronize()
            assert ws.intact() and cells.intact() and counts.intact()
            assert counts.get(np.int32).tolist() == full_counts, (n, max_cells)
            m = min(full_counts[0], max_cells)
            got = cells.get(np.int32).reshape(max_cells, 2)
            assert np.array_equal(got[:m], full_cells[:m]), (n, max_cells)
            assert (cells.get(np.uint8)[8 * m:] == GUARD_BYTE).all()             # nothing is written past the cells there are
    # the planner's own conversion puts the same Gaussians into the same cells
    from planning.astar import AstarPlanner
    p = AstarPlanner(device=gpu, cell_size=cell)
    p.grid_dim = np.array([W, H])
    p.map_center = torch.tensor(center, dtype=torch.float64, device=gpu)
    p.occ_map = torch.zeros((3, H, W), device=gpu)
    pts = _cloud(rng, W, H, cell, center, 300)
    world = p.build_object_frontiers(torch.from_numpy(pts).to(gpu))
    want_cells, _ = gc.np_object_cells(W, H, cell, center, pts, 3, W * H)
    want = (want_cells.astype(np.int64) - np.array([[W // 2, H // 2]])) * cell + np.asarray(center)[None, :]
    assert world.dtype == np.float64 and np.array_equal(world, want)
    assert p.build_object_frontiers(torch.zeros((0, 3), device=gpu)) is None and p.build_object_frontiers(None) is None
    assert p.build_object_frontiers(torch.from_numpy(pts[:3]).to(gpu)) is None                   # no cell with more than 3


# ---- fr_occ_grid_candidates ------------------------------------------------------------------------------------------------------------

def test_grid_candidates_match_the_restatement(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    W, H, cell, center = 97, 96, 0.05, (0.37, -0.21)
    cfg = _cfg(W, H, cell, center)
    rng = np.random.default_rng(5)
    eroded = np.zeros((H, W), np.uint8)
    eroded[20:80, 15:70] = 1
    eroded[40:50, :] = 0
    d_eroded = torch.from_numpy(eroded).to(gpu)
    cells = np.stack([rng.integers(30, 60, 9), rng.integers(30, 60, 9)], axis=1).astype(np.int32)     # (col, row)
    d_cells = torch.from_numpy(cells).to(gpu)
    centers_of_cells = gc.cells_to_world(cells, W, H, cell, center)
    float_centers = (rng.uniform(-0.8, 0.8, (5, 2)) + np.asarray(center)).astype(np.float32)
    d_float = torch.from_numpy(float_centers).to(gpu)
    differing = 0
    for K in (1, 33, 138, 139, 300):
        for bins in (1, 6):
            for step_deg in (360.0, 15.0):
                for sqrt_area in (0, 1):
                    for source in ("float", "cells"):
                        n_theta = gc.n_theta_of(step_deg)
                        seed = int(rng.integers(0, 2 ** 31))
                        c2w, keep = _Guarded(64 * K, gpu), _Guarded(K, gpu)
                        if source == "float":
                            args, centers = (d_float.data_ptr(), 5, None, None), float_centers
                        else:
                            # 7 of the 9 cells are there, as the device count says; the buffer has room for all 9
                            n_dev = torch.tensor([7, 123], dtype=torch.int32, device=gpu)
                            args, centers = (None, 9, d_cells.data_ptr(), n_dev.data_ptr()), centers_of_cells[:7]
                        _lib.check(lib.fr_occ_grid_candidates(ctypes.byref(cfg), *args, K, 0.3, 1.9, n_theta, bins, sqrt_area, 0.4, seed,
                                                              d_eroded.data_ptr(), 40, c2w.ptr, keep.ptr, _stream(gpu)), "fr_occ_grid_candidates")
                        torch.cuda.synchronize()
                        assert c2w.intact() and keep.intact()
                        got = c2w.get(np.float32).reshape(K, 4, 4)
                        want, want_keep = gc.np_grid_candidates(W, H, cell, center, centers, K, 0.3, 1.9, n_theta, bins, sqrt_area, 0.4, seed, eroded)
                        assert np.abs(got - want).max() <= 2e-6, (K, bins, step_deg, sqrt_area, source)
                        d = int((keep.get(np.uint8) != want_keep).sum())
                        assert d <= 1, (K, bins, step_deg, sqrt_area, source, d)
                        differing += d
                        # and exact on the device's own positions
                        col = ((got[:, 0, 3] - np.float32(center[0])) / np.float32(cell) + np.float32(W // 2)).astype(np.int64)
                        row = ((got[:, 2, 3] - np.float32(center[1])) / np.float32(cell) + np.float32(H // 2)).astype(np.int64)
                        inside = (col >= 0) & (col < W) & (row >= 0) & (row < H)
                        exact = np.where(inside, eroded[np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)] != 0, False)
                        assert np.array_equal(keep.get(np.uint8).astype(bool), exact)
    print(f"keep flags that differ from the restatement's own positions: {differing}")
    # 15 degrees: 23 angles, not 24 -- pose 23 is the first angle again on the next ring
    c2w = _Guarded(64 * 24, gpu)
    one = torch.tensor([[0.1, 0.2]], dtype=torch.float32, device=gpu)
    _lib.check(lib.fr_occ_grid_candidates(ctypes.byref(cfg), one.data_ptr(), 1, None, None, 24, 0.3, 1.9, 24, 6, 0, 0.4, 1, None, 40, c2w.ptr, None,
                                          _stream(gpu)), "fr_occ_grid_candidates")
    torch.cuda.synchronize()
    m = c2w.get(np.float32).reshape(24, 4, 4)
    assert np.array_equal(m[23, :3, :3], m[0, :3, :3]) and abs(float(m[23, 2, 3] - m[0, 2, 3]) - (1.9 - 0.3) / 5) < 1e-6
    # a filter on an almost empty free space keeps everything; no cell on the device: zero matrices that are not kept
    few = torch.zeros((H, W), dtype=torch.uint8, device=gpu)
    few[10:14, 10:14] = 1
    keep, c2w = _Guarded(50, gpu), _Guarded(64 * 50, gpu)
    _lib.check(lib.fr_occ_grid_candidates(ctypes.byref(cfg), d_float.data_ptr(), 5, None, None, 50, 0.3, 1.9, 24, 6, 0, 0.4, 3, few.data_ptr(), 40,
                                          c2w.ptr, keep.ptr, _stream(gpu)), "fr_occ_grid_candidates")
    torch.cuda.synchronize()
    assert keep.get(np.uint8).all()
    zero = torch.zeros((2,), dtype=torch.int32, device=gpu)
    _lib.check(lib.fr_occ_grid_candidates(ctypes.byref(cfg), None, 9, d_cells.data_ptr(), zero.data_ptr(), 50, 0.3, 1.9, 24, 6, 0, 0.4, 3, None, 40,
                                          c2w.ptr, keep.ptr, _stream(gpu)), "fr_occ_grid_candidates")
    torch.cuda.synchronize()
    assert not keep.get(np.uint8).any() and not c2w.get(np.float32).any() and c2w.intact() and keep.intact()


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------

STEP = dict(forward_step_size=0.25, turn_angle=30.)


@pytest.fixture(scope="module")
def two_rooms(gpu):
    """96 x 96 cells of 5 cm: two rooms, a wall between them with a door, unknown cells round them; the agent in the left room; 12 goals --
    in both rooms, in the wall, next to the agent, one of them twice; an object cloud in the right room.
    dict(planner, c (a case for the restatement), goal_c2ws, object_points, scene_points)"""
    from planning.astar import AstarPlanner
    H = W = 96
    label = np.zeros((H, W), np.int64)
    label[8:88, 8:88] = 2
    label[8:88, 48] = 1
    label[40:52, 48] = 2
    occ_map = np.zeros((3, H, W), np.float32)
    occ_map[0][label == 0] = 1
    occ_map[1][label == 1] = 1
    occ_map[2][label == 2] = 2
    c = dict(name="two-rooms", W=W, H=H, cell=0.05, center=(0.0, 0.0), turn=STEP["turn_angle"], step=STEP["forward_step_size"], Q=Q, cam_height=0.4,
             start=(20, 30))
    pol = gc.Policy(c)
    rng = np.random.default_rng(23)
    pos = pol.world_at(np.array([20.5, 30.5]) + rng.uniform(-0.2, 0.2, 2))
    c["agent"] = gc.cam_pose(rng.uniform(-np.pi, np.pi), pos[0], 1.1, pos[1])
    cells = [(70, 20), (30, 75), (60, 80), (46, 70), (30, 48), (30, 21), (70, 20), (15, 40), (80, 60), (2, 2), (45, 30), (12, 84)]     # (row, col)
    goal_c2ws = np.zeros((len(cells), 4, 4), np.float32)
    for g, (row, col) in enumerate(cells):
        w = pol.world_at(np.array([col, row]) + 0.5 + rng.uniform(-0.3, 0.3, 2))
        goal_c2ws[g] = gc.cam_pose(rng.uniform(-np.pi, np.pi), w[0], rng.uniform(0.2, 1.5), w[1], np.float32)
    goal_c2ws[6] = goal_c2ws[0]                                  # the same goal twice: cell and pose
    c["goals"] = np.array(cells, np.int32)
    c["goals_c2w"] = goal_c2ws
    p = AstarPlanner(device=gpu, cell_size=c["cell"], sample_view_num_object=138, sample_range_object=0.9, min_range_object=0.3)
    p.grid_dim = np.array([W, H])
    p._map_center_np = np.zeros(2)
    p.map_center = torch.from_numpy(p._map_center_np).to(gpu)
    p.cam_height = c["cam_height"]
    p.cam_pos = np.array([30, 20])
    p.occ_map = torch.from_numpy(occ_map).to(gpu)
    # the object: 40 Gaussians in each of 6 cells of the right room
    obj_cells = np.array([(70, 44), (71, 44), (72, 44), (70, 45), (71, 45), (72, 45)])                  # (col, row)
    xz = ((obj_cells[:, None, :] - (np.array([W, H]) - 1) // 2 + 0.5) * c["cell"] + rng.uniform(-0.02, 0.02, (6, 40, 2))).reshape(-1, 2)
    obj = np.stack([xz[:, 0], rng.uniform(-0.3, 0.3, len(xz)), xz[:, 1]], axis=1).astype(np.float32)
    return dict(planner=p, c=c, goal_c2ws=goal_c2ws, object_points=torch.from_numpy(obj).to(gpu), object_cells=obj_cells)


def test_plan_actions_object_equals_plan_paths_fed_to_the_restatement(gpu, two_rooms, monkeypatch):
    p, c, goal_c2ws = two_rooms["planner"], two_rooms["c"], two_rooms["goal_c2ws"]
    p.setup_start(np.array([c["start"][1], c["start"][0]]))
    paths = p.plan_paths(c["goals"])
    want = gc.np_action_planning_object_adv(c, paths_list=paths)
    assert want["margin"] > gc.MARGIN and want["yaw_margin"] > gc.YAW_MARGIN, (want["margin"], want["yaw_margin"])
    assert want["n_actions"][4] == -1 and want["n_actions"][9] == -1 and want["keep"][6] == 0 and sum(want["keep"]) >= 6        # wall, unknown, twice
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1])
    plan = p.plan_actions_object(goal_c2ws, c["agent"], **STEP)
    monkeypatch.undo()
    assert len(reads) == 1 and plan.reads == 1, reads                    # one read for the actions, none for the poses
    assert plan.w2c.is_cuda and plan.w2c.shape == (12, Q, 4, 4)
    assert plan.n_actions.tolist() == want["n_actions"] and plan.keep.tolist() == want["keep"]
    assert plan.kept_index == want["kept_index"] and plan.path_actions == want["path_actions"]
    for a, b in zip(plan.paths, paths):
        assert np.array_equal(a, b)
    vg, pa, arr = plan.triple()
    w2c = plan.w2c.cpu().numpy()
    for k, g in enumerate(want["kept_index"]):
        n = want["n_actions"][g]
        assert np.array_equal(vg[k], goal_c2ws[g]) and np.array_equal(arr[k], want["paths_arr"][k]) and arr[k].dtype == np.int32
        assert len(plan.map_path[k]) == len(plan.world_path[k]) == want["actions"][g].count(1)
        assert gc.ulp32(w2c[g, :n], np.linalg.inv(want["c2w"][g]).astype(np.float32)).max() <= 1
        assert not w2c[g, n:].any()
    # the round's first half as the reference returns it
    from fisher_rast import plan_round
    triple = plan_round.action_planning_object_adv(p, goal_c2ws, c["agent"], None, 3, **STEP)
    assert triple[1] == want["path_actions"] and len(triple[0]) == len(triple[2]) == len(want["kept_index"])
    # a path longer than the first call's room repeats both calls and the read, and gives the same
    p.PLAN_MAX_LEN = 2
    again = p.plan_actions_object(goal_c2ws, c["agent"], **STEP)
    del p.PLAN_MAX_LEN
    assert again.reads == 2 and again.path_actions == plan.path_actions and torch.equal(again.w2c, plan.w2c)
    assert all(np.array_equal(a, b) for a, b in zip(again.paths_arr, plan.paths_arr))


def _stub_pose_eval(calls):
    """scores that fall with the distance from a fixed point: deterministic, with a strict order"""
    def pose_eval(poses, random_gaussian_params, criterion=None):
        calls.append((tuple(poses.shape), random_gaussian_params, criterion))
        xz = poses[:, [0, 2], 3].cpu()
        return 10.0 - torch.linalg.norm(xz - torch.tensor([1.4, -0.3]), dim=1), poses
    return pose_eval


def test_global_object_planning_on_two_rooms(gpu, two_rooms):
    p = two_rooms["planner"]
    p.candidate_seed = 11
    calls = []
    poses, scores, rgp, centres = p.global_object_planning(_stub_pose_eval(calls), two_rooms["object_points"], None, None, expansion=1, visualize=True,
                                                           agent_pose=np.array([0.0, 0.4, 0.0]), criterion="topt")
    assert rgp is None and len(calls) == 1 and calls[0][1] is None and calls[0][2] == "topt"
    # the object's cells, as world positions in np.where order
    want_centres = (two_rooms["object_cells"][np.lexsort((two_rooms["object_cells"][:, 0], two_rooms["object_cells"][:, 1]))] - 48) * 0.05
    assert np.allclose(centres.cpu().numpy(), want_centres, atol=1e-12)
    # the candidates: the sorted grid around those cells, the ones in the eroded free space -- from the cells left on the device
    n_cand = calls[0][0][0]
    eroded = p._eroded_free(None, 10)
    c2w, keep = p._grid_candidates(None, 1, eroded=eroded, seed=11, cells_dev=p._object_cells_dev)
    assert 0 < n_cand == int(keep.sum()) < p.K_object and p.last_widenings == 1
    from_host, _ = p._grid_candidates(torch.from_numpy(want_centres).to(gpu), 1, eroded=eroded, seed=11)     # the same centres, by way of the host
    assert float((from_host - c2w).abs().max()) <= 2e-6
    # the top 20 by score, in descending order
    all_scores, _ = _stub_pose_eval([])(c2w[keep], None)
    order = torch.argsort(all_scores, descending=True)[:20]
    assert poses.shape == (20, 4, 4) and torch.equal(poses, c2w[keep][order.to(gpu)]) and torch.equal(scores, all_scores[order])
    assert p.previous_candidates is poses
    # frontier mode without an object: nothing to do; with an evaluation: the random poses of the free space
    assert p.global_object_planning(None, torch.zeros((0, 3), device=gpu), None) == (None, None, None)
    calls.clear()
    poses, scores, _, centres = p.global_object_planning(_stub_pose_eval(calls), None, None, None, agent_pose=np.array([0.0, 0.4, 0.0]))
    assert centres is None and calls[0][0][0] > 20 and poses.shape == (20, 4, 4)
    # the scene round on the same stages
    calls.clear()
    p.frontier_select_method = "largest"
    poses, scores, rgp = p.global_planning(lambda c, r: _stub_pose_eval(calls)(c, r), None, None, agent_pose=np.array([0.0, 0.4, 0.0]))
    assert rgp is None and poses.shape[0] == scores.shape[0] <= 20 and bool((scores[:-1] >= scores[1:]).all())
    p.frontier_select_method = "vlm"
    with pytest.raises(ValueError, match="vlm"):
        p.global_object_planning(None, two_rooms["object_points"])
    p.frontier_select_method = "combined"


def test_plan_best_object_path_choice_and_shapes(gpu, two_rooms):
    from fisher_rast import plan_round
    p, c = two_rooms["planner"], two_rooms["c"]
    p.candidate_seed = 11
    calls = []
    obj_slam = types.SimpleNamespace(gaussian_points=two_rooms["object_points"], pose_eval=_stub_pose_eval(calls))
    slam = types.SimpleNamespace(gaussian_points=None)
    for w_end in (0.0, 0.5):
        cfg = dict(STEP, object_path_end_weight=w_end)
        res = plan_round.plan_best_object_path(obj_slam, slam, p, c["agent"], 1, 0, cfg, "fisher")
        best_path, best_map_path, best_goal, best_world_path, best_global_path, global_points, EIGs = res
        plan = res.plan
        assert global_points.shape == (20, 4, 4) and EIGs.shape == (20,) and bool((EIGs[:-1] >= EIGs[1:]).all())
        assert len(res.totals) == len(res.scored) == min(len(plan.kept_index), plan_round.MAX_SCORED_PATHS) >= 3
        want = [w_end * float(EIGs[i]) if w_end > 0 else float(EIGs[i]) / len(plan.path_actions[i]) for i in res.scored]
        assert np.allclose(res.totals, want, rtol=1e-12, atol=0)
        k = res.best_index
        assert k == res.scored[int(np.argmax(res.totals))] and max(res.totals) > -1
        assert best_path == plan.path_actions[k] and all(isinstance(a, int) for a in best_path) and 0 < len(best_path) <= 200
        assert best_goal.shape == (4, 4) and np.array_equal(best_goal, global_points[plan.kept_index[k]])
        assert best_global_path.ndim == 2 and best_global_path.shape[1] == 2 and best_global_path.dtype == np.int32
        assert len(best_map_path) == len(best_world_path) == best_path.count(1)
        assert all(m.shape == (2,) and w.shape == (2,) for m, w in zip(best_map_path, best_world_path))
