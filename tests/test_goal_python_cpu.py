"""The object round's Python layer on the CPU, on a stand-in library (the g++ harness behind the entry points, the planner's tensors on the
host), as tests/test_action_plan_cpu.py does for plan_actions: PathPlanOps.plan_actions_object (one host read, the repeat for a long
path, the pruned paths as paths_arr), GoalSelectOps.global_object_planning / global_planning (the widening loop, the filter fused into
the candidate launch, the random poses without a frontier, the top-20 cut, previous_candidates), plan_round.plan_best_object_path (the
closed-form "fisher" value, the 21-path cap, the first maximum above the floor); the grafts' signatures against the reference's."""
import ast
import ctypes
import json
import os
import types

import numpy as np
import pytest
import torch

import goal_cases as gc


@pytest.fixture(scope="module")
def harness():
    return gc.build_harness()


_CACHE = {}


def _computed(h, family):
    if family not in _CACHE:
        c = gc.make_case(family)
        _CACHE[family] = (c, gc.np_action_planning_object_adv(c))
    return _CACHE[family]


def _as(ptr, dtype, shape):
    return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(dtype)), shape)


class _StandInLib:
    """fr_plan_paths hands out a case's paths (-1 where one does not fit max_len); fr_plan_actions_object, fr_occ_object_cells and
    fr_occ_grid_candidates are the g++ harness; the keep flags of the candidates are scripted per launch"""

    def __init__(self, h, c=None, keep_script=()):
        self.h, self.c, self.calls, self.keep_script = h, c, [], list(keep_script)

    def fr_occ_workspace_bytes(self, cfg):
        return 4096

    def fr_plan_paths(self, cfg, field, occ, sy, sx, goals, G, shortcut, paths, max_len, lengths, stream):
        c = self.c
        self.calls.append(("fr_plan_paths", max_len))
        assert G == len(c["lengths"]) and (sy, sx) == (c["start"][1], c["start"][0])
        out_p, out_n = _as(paths, ctypes.c_int32, (G, max_len, 2)), _as(lengths, ctypes.c_int32, (G,))
        for g, n in enumerate(c["lengths"]):
            if n > max_len:
                out_n[g] = -1
            else:
                out_n[g] = max(int(n), 0)
                out_p[g, :max(int(n), 0)] = c["paths"][g, :max(int(n), 0)]
        return 0

    def fr_plan_actions_object(self, cfg, paths, max_len, lengths, goals, poses, G, agent, height, step, turn, cell, actions, n, keep, w2c, xz, cells,
                               pruned, plen, stream):
        self.calls.append(("fr_plan_actions_object", max_len))
        o = cfg._obj
        hit = np.zeros(G, np.int32)
        self.h.frg_h_plan_object(o.grid_w, o.grid_h, cell, o.center_x, o.center_z, paths, max_len, lengths, goals, poses, G, ctypes.addressof(agent), height,
                                 step, turn, actions, n, keep, w2c, xz, cells, pruned, plen, hit.ctypes.data)
        assert not hit.any()
        return 0

    def fr_occ_object_cells(self, cfg, points, n, min_count, cells, max_cells, counts, ws, ws_bytes, stream):
        self.calls.append(("fr_occ_object_cells", n, min_count))
        o = cfg._obj
        self.h.frg_h_object_cells(o.grid_w, o.grid_h, o.cell_size, o.center_x, o.center_z, points, n, min_count, cells, max_cells, counts)
        return 0

    def fr_occ_erode(self, cfg, src, dst, ksize, stream):
        self.calls.append(("fr_occ_erode", ksize))
        o = cfg._obj
        ctypes.memmove(dst, src, o.grid_w * o.grid_h)
        return 0

    def _keep(self, K, keep):
        flags = self.keep_script.pop(0) if self.keep_script else np.ones(K, np.uint8)
        _as(keep, ctypes.c_uint8, (K,))[:] = flags

    def fr_occ_grid_candidates(self, cfg, centers, n_centers, cells, n_dev, K, lo, hi, n_theta, bins, sqrt_area, h, seed, eroded, min_free, c2w, keep, stream):
        o = cfg._obj
        self.calls.append(("fr_occ_grid_candidates", "cells" if cells else "float", n_centers, K, round(hi, 6), n_theta, bins, sqrt_area, eroded is not None, min_free))
        if cells:
            n = min(int(_as(n_dev, ctypes.c_int32, (1,))[0]), n_centers)
            held = gc.cells_to_world(_as(cells, ctypes.c_int32, (n, 2)), o.grid_w, o.grid_h, o.cell_size, (o.center_x, o.center_z))
            centers, n_centers = held.ctypes.data, n
        self.h.frg_h_grid(centers, n_centers, K, lo, hi, n_theta, bins, sqrt_area, h, seed, c2w)
        self._keep(K, keep)
        return 0

    def fr_occ_ring_candidates(self, cfg, centers, n_centers, K, lo, hi, h, seed, eroded, min_free, c2w, keep, stream):
        self.calls.append(("fr_occ_ring_candidates", n_centers, K, round(hi, 6), eroded is not None, min_free))
        out = _as(c2w, ctypes.c_float, (K, 4, 4))
        out[:] = np.eye(4, dtype=np.float32)
        out[:, 0, 3] = np.arange(K) * 0.01 + hi                     # a pose's x tells the launch and the index
        self._keep(K, keep)
        return 0


def _stand_in_planner(monkeypatch, fake, W, H, cell, center, cam_height=0.4, **kw):
    from fisher_rast import _lib
    from planning import AstarPlanner
    monkeypatch.setattr(_lib, "load", lambda: fake)
    pl = AstarPlanner(device="cpu", cell_size=cell, **kw)
    pl.grid_dim = np.array([W, H])
    pl.map_center = torch.tensor(center, dtype=torch.float32)
    pl.cam_height = cam_height
    pl.occ_map = torch.zeros((3, H, W))
    pl._stream = lambda: None
    return pl


def _plan_ready(pl, c):
    sx, sz = c["start"]
    pl._plan = dict(cfg=pl._occ_cfg(), start=(sz, sx), field=torch.zeros(1, dtype=torch.int64), occ_plan=torch.zeros(1, dtype=torch.uint8))
    reads = []
    pl._plan_read = lambda t: (reads.append(tuple(t.shape)), t.cpu().numpy())[1]
    return reads


# ---- plan_actions_object -----------------------------------------------------------------------------------------------------------------

def _goals_at_finish(c):
    """cases whose goal poses convert to the case's own goal cells (the wrapper derives the cells from the poses)"""
    pol = gc.Policy(c)
    return all(pol.convert_to_map(pose[[0, 2], 3])[[1, 0]].tolist() == c["goals"][g].tolist() for g, pose in enumerate(c["goals_c2w"]))


@pytest.mark.parametrize("family", ["odd-grid", "all-pruned", "at-goal", "all-without-path", "cap"])
def test_plan_actions_object_host_logic_on_a_stand_in_library(monkeypatch, harness, family):
    c, want = _computed(harness, family)
    assert _goals_at_finish(c)
    fake = _StandInLib(harness, c)
    pl = _stand_in_planner(monkeypatch, fake, c["W"], c["H"], c["cell"], c["center"], c["cam_height"])
    reads = _plan_ready(pl, c)
    plan = pl.plan_actions_object(c["goals_c2w"], c["agent"], forward_step_size=c["step"], turn_angle=c["turn"])
    assert len(reads) == 1 and plan.reads == 1 and [n for n, _ in fake.calls] == ["fr_plan_paths", "fr_plan_actions_object"]
    assert plan.kept_index == want["kept_index"] and plan.path_actions == want["path_actions"]
    assert plan.n_actions.tolist() == want["n_actions"] and plan.keep.tolist() == want["keep"]
    vg, pa, arr = plan.triple()
    assert len(vg) == len(pa) == len(arr) == len(want["kept_index"])
    for k, g in enumerate(want["kept_index"]):
        assert np.array_equal(vg[k], c["goals_c2w"][g])
        assert np.array_equal(arr[k], want["paths_arr"][k]) and arr[k].dtype == np.int32            # the PRUNED path
        assert len(plan.map_path[k]) == len(plan.world_path[k]) == want["actions"][g].count(1)
    for g, pr in enumerate(want["pruned"]):
        assert np.array_equal(plan.pruned[g], pr if pr is not None else np.zeros((0, 2)))
    assert plan.w2c.shape == (len(c["lengths"]), 200, 4, 4) and plan.kept_w2c().shape[0] == len(want["kept_index"])
    assert [len(p) for p in plan.paths] == [max(int(n), 0) for n in c["lengths"]]
    assert all(len(a) > 0 for a in plan.path_actions)                                                # an empty list is dropped


def test_plan_actions_object_repeats_once_for_a_long_path_and_validates(monkeypatch, harness):
    c, want = _computed(harness, "lanes")
    assert _goals_at_finish(dict(c, goals_c2w=c["goals_c2w"][:5], goals=c["goals"][:5]))
    # the goal of the sixth path is not at its path's end: the wrapper would plan to another cell, so the first five go through it
    c = dict(c, paths=c["paths"][:5], lengths=c["lengths"][:5], goals=c["goals"][:5], goals_c2w=c["goals_c2w"][:5])
    want = gc.np_action_planning_object_adv(c)
    fake = _StandInLib(harness, c)
    pl = _stand_in_planner(monkeypatch, fake, c["W"], c["H"], c["cell"], c["center"], c["cam_height"])
    reads = _plan_ready(pl, c)
    pl.PLAN_MAX_LEN = 64                                       # the paths have up to 130 points
    kw = dict(forward_step_size=c["step"], turn_angle=c["turn"])
    plan = pl.plan_actions_object(torch.from_numpy(c["goals_c2w"]), torch.from_numpy(c["agent"]), **kw)
    room = c["W"] * c["H"] + 1
    assert fake.calls == [("fr_plan_paths", 64), ("fr_plan_actions_object", 64), ("fr_plan_paths", room), ("fr_plan_actions_object", room)]
    assert plan.reads == 2 == len(reads) and plan.path_actions == want["path_actions"]
    assert all(np.array_equal(a, b) for a, b in zip(plan.paths_arr, want["paths_arr"]))
    # no goals: nothing is called or read
    fake.calls.clear()
    empty = pl.plan_actions_object(np.zeros((0, 4, 4), np.float32), c["agent"], **kw)
    assert empty.triple() == ([], [], []) and empty.reads == 0 and not fake.calls and empty.w2c.shape == (0, 200, 4, 4)
    for bad in (dict(kw, forward_step_size=0.0), dict(kw, turn_angle=-10.)):
        with pytest.raises(ValueError):
            pl.plan_actions_object(c["goals_c2w"], c["agent"], **bad)
    with pytest.raises(ValueError, match="4 x 4"):
        pl.plan_actions_object(c["goals_c2w"], c["agent"][:3], **kw)
    moved = c["agent"].copy()
    moved[0, 3] += 3 * c["cell"]
    with pytest.raises(ValueError, match="setup_start"):
        pl.plan_actions_object(c["goals_c2w"], moved, **kw)
    with pytest.raises(TypeError):
        pl.plan_actions_object(c["goals_c2w"], c["agent"], queue_size=30, **kw)                     # the planning queue does not cut these lists
    assert not fake.calls


def test_install_grafts_the_object_round():
    from planning import astar
    keep = lambda self, poses, *a: None
    cls = type("RefPlanner", (), {"pose_eval": keep})
    astar.PathPlanOps.install(cls)
    astar.GoalSelectOps.install(cls)
    assert cls.plan_actions_object is astar.PathPlanOps.__dict__["plan_actions_object"] and cls._action_inputs is astar.PathPlanOps.__dict__["_action_inputs"]
    for name in ("build_object_frontiers", "generate_candidate_adv_object", "global_planning", "global_object_planning", "_select_goals"):
        assert getattr(cls, name) is astar.GoalSelectOps.__dict__[name]
    assert cls.pose_eval is keep                                  # the reference class keeps its own
    assert issubclass(astar.AstarPlanner, astar.GoalSelectOps)
    # OccupancyOps.install is as it was: the new grafts have their own
    assert "build_object_frontiers" not in astar.OccupancyOps.__dict__


# ---- global_object_planning / global_planning ------------------------------------------------------------------------------------------------

W = H = 96
CELL, CENTER = 0.05, (0.0, 0.0)


def _object_cloud():
    """40 Gaussians in each of 6 cells, 3 in a seventh: (points float32 [n, 3], the six cells (col, row) in np.where order)"""
    rng = np.random.default_rng(4)
    cells = np.array([(70, 44), (71, 44), (72, 44), (70, 45), (71, 45), (72, 45)])
    xz = ((cells[:, None, :] - (W - 1) // 2 + 0.5) * CELL + rng.uniform(-0.02, 0.02, (6, 40, 2))).reshape(-1, 2)
    lone = ((np.array([[20, 20]]) - (W - 1) // 2 + 0.5) * CELL).repeat(3, axis=0)
    xz = np.concatenate([xz, lone])
    return np.stack([xz[:, 0], rng.uniform(-0.3, 0.3, len(xz)), xz[:, 1]], axis=1).astype(np.float32), cells


def _goal_planner(monkeypatch, harness, keep_script=(), frontier=None, **kw):
    fake = _StandInLib(harness, keep_script=keep_script)
    pl = _stand_in_planner(monkeypatch, fake, W, H, CELL, CENTER, sample_view_num_object=50, sample_range_object=0.8, min_range_object=0.3,
                           sample_view_num=40, sample_range=1.0, min_range=0.2, **kw)
    free = np.ones((H, W), np.uint8)

    def build_frontiers(gaussian_points=None):
        fake.calls.append(("build_frontiers", None if gaussian_points is None else tuple(gaussian_points.shape)))
        pl._free_space_dev = torch.from_numpy(free)
        return frontier, free
    pl.build_frontiers = build_frontiers
    randoms = torch.eye(4).repeat(7, 1, 1)
    randoms[:, 0, 3] = 100 + torch.arange(7)
    pl.sample_random_candidate = lambda agent_pos, free_space, sample_range=1., sample_size=100, seed=None: (
        fake.calls.append(("sample_random_candidate", round(sample_range, 6), sample_size)), randoms)[1]
    pl.candidate_seed = 5
    return pl, fake


def _score_by_x(calls):
    def fn(poses, random_gaussian_params, criterion=None):
        calls.append((tuple(poses.shape), random_gaussian_params, criterion))
        return poses[:, 0, 3].clone() * -1.0 + torch.arange(poses.shape[0]) * 1e-4, poses
    return fn


def test_global_object_planning_widens_filters_and_cuts_to_the_top_20(monkeypatch, harness):
    pts, cells = _object_cloud()
    first = np.zeros(50, np.uint8)                               # nothing in the free space at expansion 1
    second = (np.arange(50) % 5 != 0).astype(np.uint8)           # 40 of 50 at expansion 1.5
    pl, fake = _goal_planner(monkeypatch, harness, keep_script=[first, second])
    calls = []
    scene = torch.zeros((9, 3))
    poses, scores, rgp, centres = pl.global_object_planning(_score_by_x(calls), torch.from_numpy(pts), scene, None, expansion=1, visualize=True,
                                                            agent_pose=np.array([0., 0.4, 0.]), criterion="dopt")
    names = [k[0] for k in fake.calls]
    assert names == ["build_frontiers", "fr_occ_object_cells", "fr_occ_erode", "fr_occ_grid_candidates", "fr_occ_grid_candidates"]
    assert fake.calls[0][1] == (9, 3) and fake.calls[1][1:] == (len(pts), 3) and fake.calls[2][1] == 10                 # the scene's points; count > 3
    # the candidates come from the cells on the device, 24 -> 23 angles x 6 rings, the filter in the launch, the radius widened by 1.5
    assert fake.calls[3][1:] == ("cells", W * H, 50, 0.8, 24, 6, 0, True, 40) and fake.calls[4][1:] == ("cells", W * H, 50, 1.2, 24, 6, 0, True, 40)
    assert pl.last_widenings == 2 and rgp is None
    want_centres = (cells - 48) * CELL
    assert np.allclose(centres.numpy(), want_centres, atol=1e-12) and centres.dtype == torch.float64
    # one evaluation over the kept poses; the top 20 by argsort(descending); previous_candidates
    assert len(calls) == 1 and calls[0] == ((40, 4, 4), None, "dopt")
    c2w = np.zeros((50, 4, 4), np.float32)
    held = gc.cells_to_world(cells, W, H, CELL, CENTER)
    harness.frg_h_grid(held.ctypes.data, 6, 50, 0.3, np.float32(1.2), 24, 6, 0, 0.4, 6, c2w.ctypes.data)               # the second launch's seed
    kept = torch.from_numpy(c2w[second.astype(bool)])
    all_scores, _ = _score_by_x([])(kept, None)
    order = torch.argsort(all_scores, descending=True)[:20]
    assert poses.shape == (20, 4, 4) and torch.equal(poses, kept[order]) and torch.equal(scores, all_scores[order])
    assert pl.previous_candidates is poses
    # centering: one float centre, the mean
    pl2, fake2 = _goal_planner(monkeypatch, harness, centering=True)
    _, _, _, centre = pl2.global_object_planning(_score_by_x([]), torch.from_numpy(pts), None)
    assert fake2.calls[-1][1:4] == ("float", 1, 50) and np.allclose(centre.numpy(), want_centres.mean(axis=0, keepdims=True), atol=1e-12)
    # the widening loop ends
    pl3, fake3 = _goal_planner(monkeypatch, harness, keep_script=[np.zeros(50, np.uint8)] * 100)
    pl3.MAX_WIDENINGS = 4
    with pytest.raises(RuntimeError, match="widenings"):
        pl3.global_object_planning(_score_by_x([]), torch.from_numpy(pts), None)
    assert [k[0] for k in fake3.calls].count("fr_occ_grid_candidates") == 4


def test_global_object_planning_without_object_cells(monkeypatch, harness):
    pl, fake = _goal_planner(monkeypatch, harness)
    # frontier mode: nothing to return, nothing sampled
    assert pl.global_object_planning(None, None, None) == (None, None, None)
    assert pl.global_object_planning(None, torch.zeros((0, 3)), None) == (None, None, None)
    pts, _ = _object_cloud()
    assert pl.global_object_planning(None, torch.from_numpy(pts[-3:]), None) == (None, None, None)                     # 3 in a cell is not more than 3
    assert "fr_occ_grid_candidates" not in [k[0] for k in fake.calls]
    # with an evaluation: a proposal's centres if there is one, and the random poses of the free space
    calls = []
    proposal = lambda K, h: np.array([[0.5, 0.25]]) if (K, h) == (50, 0.4) else None
    poses, scores, rgp, centres = pl.global_object_planning(_score_by_x(calls), None, None, proposal, expansion=2, agent_pose=np.array([0., 0.4, 0.]))
    assert calls[0][0] == (57, 4, 4) and poses.shape == (20, 4, 4) and centres.shape == (1, 2)
    grid = [k for k in fake.calls if k[0] == "fr_occ_grid_candidates"][-1]
    assert grid[1:5] == ("float", 1, 50, 1.6)
    assert [k for k in fake.calls if k[0] == "sample_random_candidate"][-1][1:] == (6.0, 1200)      # 2 x and 400 x the widened expansion
    calls.clear()
    poses, scores, rgp, centres = pl.global_object_planning(_score_by_x(calls), None, None, None, agent_pose=np.array([0., 0.4, 0.]))
    assert calls[0][0] == (7, 4, 4) and poses.shape == (7, 4, 4) and centres is None
    # no evaluation function but object cells: every pose scores 1
    poses, scores, _, _ = pl.global_object_planning(None, torch.from_numpy(pts), None)
    assert poses.shape == (20, 4, 4) and torch.equal(scores, torch.ones(20))
    pl.frontier_select_method = "vlm"
    with pytest.raises(ValueError, match="vlm"):
        pl.global_object_planning(None, torch.from_numpy(pts), None)
    with pytest.raises(ValueError, match="vlm"):
        pl.global_planning(None)


def test_global_planning_on_the_ring(monkeypatch, harness):
    frontier = np.array([[0.5, 0.25], [0.6, 0.25]])
    first = np.zeros(40, np.uint8)
    second = np.ones(40, np.uint8)
    second[::4] = 0
    pl, fake = _goal_planner(monkeypatch, harness, keep_script=[first, second], frontier=frontier)
    calls = []
    pts = torch.zeros((5, 3))
    poses, scores, rgp = pl.global_planning(lambda c, r: _score_by_x(calls)(c, r), pts, None, expansion=1, visualize=True, agent_pose=np.array([0., 0.4, 0.]))
    assert [k[0] for k in fake.calls] == ["build_frontiers", "fr_occ_erode", "fr_occ_ring_candidates", "fr_occ_ring_candidates"]
    assert fake.calls[2][1:] == (2, 40, 1.0, True, 40) and fake.calls[3][1:] == (2, 40, 1.5, True, 40)
    assert calls[0][0] == (30, 4, 4) and rgp is None and poses.shape == (20, 4, 4) and bool((scores[:-1] >= scores[1:]).all())
    assert pl.previous_candidates is poses and "sample_random_candidate" not in [k[0] for k in fake.calls]
    # frontier mode without a frontier
    pl2, fake2 = _goal_planner(monkeypatch, harness)
    assert pl2.global_planning(None) == (None, None, None)
    # no frontier, an evaluation: the random poses alone
    calls.clear()
    poses, scores, _ = pl2.global_planning(lambda c, r: _score_by_x(calls)(c, r), None, None, agent_pose=np.array([0., 0.4, 0.]))
    assert calls[0][0] == (7, 4, 4) and [k for k in fake2.calls if k[0] == "sample_random_candidate"][-1][1:] == (2.0, 400)
    # add_random_gaussians: the reference's distribution, 200 per cell; global_object_planning discards them
    pl3, _ = _goal_planner(monkeypatch, harness, frontier=frontier, add_random_gaussians=True)
    seen = []
    poses, scores, rgp = pl3.global_planning(lambda c, r: (seen.append(r), _score_by_x([])(c, r))[1], None)
    assert rgp is seen[0] and rgp["means3D"].shape == (400, 3) and rgp["rotations"][:, 0].eq(1).all() and rgp["shs"].shape == (400, 1, 3)
    y = rgp["means3D"][:, 1]
    assert float(y.min()) >= pl3.cam_height - 1.0 and float(y.max()) <= pl3.cam_height and float(rgp["opacity"].min()) >= 1e-3
    assert float(rgp["scales"].max()) <= CELL * 0.05 and float((rgp["means3D"][:200, [0, 2]] - torch.tensor(frontier[0]).float()).abs().max()) <= CELL + 1e-6
    pts, _ = _object_cloud()
    assert pl3.global_object_planning(_score_by_x([]), torch.from_numpy(pts), None)[2] is None


def test_generate_candidate_adv_object_modes(monkeypatch, harness):
    pl, fake = _goal_planner(monkeypatch, harness)
    centre = torch.tensor([[0.5, 0.25]])
    a = pl.generate_candidate_adv_object(centre, expansion=2)
    assert a.shape == (50, 4, 4) and fake.calls[-1] == ("fr_occ_ring_candidates", 1, 50, 1.6, False, 40)           # mode="random": the ring
    b = pl.generate_candidate_adv_object(centre, 1, mode="sorted", theta_step_deg=360.0, radial_bins=0, radial_spacing="sqrt_area")
    assert b.shape == (50, 4, 4) and fake.calls[-1] == ("fr_occ_grid_candidates", "float", 1, 50, 0.8, 1, 1, 1, False, 40)
    with pytest.raises(ValueError, match="mode"):
        pl.generate_candidate_adv_object(centre, mode="spiral")
    with pytest.raises(ValueError, match="theta_step_deg"):
        pl.generate_candidate_adv_object(centre, mode="sorted", theta_step_deg=0.0)


# ---- plan_best_object_path -------------------------------------------------------------------------------------------------------------------

class _FakePlanner:
    """global_object_planning hands out 25 goals with known scores; plan_actions_object keeps every goal but the third, each with a list
    of its own"""
    cam_height = 0.4

    def __init__(self, lengths):
        self.lengths, self.calls = lengths, []

    def global_object_planning(self, fn, gaussian_points, gaussian_points_scene, goal_proposal_fn, expansion=1, visualize=True, agent_pose=None, criterion=None):
        self.calls.append(("global_object_planning", fn, gaussian_points, gaussian_points_scene, goal_proposal_fn, expansion, visualize, criterion))
        n = len(self.lengths)
        poses = torch.eye(4).repeat(n, 1, 1)
        poses[:, 0, 3] = torch.arange(n).float()
        scores = torch.tensor([(7 * k) % n + 1.0 for k in range(n)])           # not sorted
        return poses, scores, None, torch.zeros((1, 2))

    def _plan_to_map(self, xz):
        return np.array([3, 4])

    def setup_start(self, start, gaussian_points, t):
        self.calls.append(("setup_start", start.tolist(), gaussian_points, t))

    def plan_actions_object(self, goal_c2ws, agent_c2w, *, forward_step_size, turn_angle):
        from planning.astar import ObjectActionPlan
        self.calls.append(("plan_actions_object", forward_step_size, turn_angle))
        G, Q = len(goal_c2ws), 200
        n = np.array(self.lengths, np.int32)
        keep = (n > 0).astype(np.uint8)
        actions = np.zeros((G, Q), np.uint8)
        for g in range(G):
            actions[g, :max(n[g], 0)] = 1 + (np.arange(max(n[g], 0)) + g) % 3
        pruned = [np.array([[g, 0], [g, 1]], np.int32) for g in range(G)]
        return ObjectActionPlan(goal_c2ws, [np.zeros((2, 2), np.int64)] * G, pruned, n, keep, actions, np.zeros((G, Q, 2), np.int32),
                                np.zeros((G, Q, 2)), torch.zeros((G, Q, 4, 4)), np.zeros((G, 2), np.int64), reads=1)


def test_plan_best_object_path_fisher_value_cap_and_choice(monkeypatch):
    from fisher_rast import path_eval, plan_round
    lengths = [4, 9, 0, 2, 7] + [5 + k for k in range(20)]
    lengths[6] = -1
    obj_slam = types.SimpleNamespace(gaussian_points="object", pose_eval="pose_eval", pose_eval_popgs="pose_eval_popgs", pose_proposal="proposal",
                                     compute_H_train=lambda *a: pytest.fail("no Hessian is launched for criteria fisher"),
                                     compute_H_train_popgs=lambda: "H_popgs")
    slam = types.SimpleNamespace(gaussian_points="scene")
    agent = np.eye(4)
    agent[:3, 3] = (0.1, 1.1, -0.2)
    monkeypatch.setattr(path_eval, "evaluate_paths_popgs", lambda *a, **k: pytest.fail("criteria fisher does not go to the POp-GS evaluation"))
    for w_end in (0.0, 0.5):
        pl = _FakePlanner(lengths)
        res = plan_round.plan_best_object_path(obj_slam, slam, pl, agent, 3, 17, dict(forward_step_size=0.25, turn_angle=30., object_path_end_weight=w_end), "Fisher")
        assert pl.calls[0][1:] == ("pose_eval", "object", "scene", "proposal", 3, False, None)
        assert pl.calls[1] == ("setup_start", [4, 3], "scene", 17) and pl.calls[2] == ("plan_actions_object", 0.25, 30.)
        best_path, best_map_path, best_goal, best_world_path, best_global_path, global_points, EIGs = res
        assert len(res) == 7 and EIGs.tolist() == sorted(EIGs.tolist(), reverse=True) and global_points[:, 0, 3].tolist() == [float((18 * (e - 1)) % 25) for e in EIGs]
        plan = res.plan
        assert len(plan.kept_index) == 23 and res.scored == list(range(21)) and len(res.totals) == 21            # 21 paths at the most
        # the i-th KEPT path with EIGs[i], as the reference zips them; the closed form
        want = [w_end * float(EIGs[i]) if w_end > 0 else float(EIGs[i]) / lengths[plan.kept_index[i]] for i in range(21)]
        assert res.totals == want
        k = int(np.argmax(want))
        assert res.best_index == k and best_path == plan.path_actions[k] and np.array_equal(best_goal, global_points[plan.kept_index[k]])
        assert np.array_equal(best_global_path, plan.pruned[plan.kept_index[k]]) and len(best_map_path) == len(best_world_path) == best_path.count(1)
    # nothing above the floor of -1: no best path
    pl = _FakePlanner(lengths)
    pl.global_object_planning = lambda *a, **k: (torch.eye(4).repeat(25, 1, 1), -5.0 - torch.arange(25.), None, None)
    res = plan_round.plan_best_object_path(obj_slam, slam, pl, agent, 1, 0, dict(forward_step_size=0.25, turn_angle=30., object_path_end_weight=1.0), "fisher")
    assert res[:5] == (None, None, None, None, None) and res.best_index is None and len(res.totals) == 21
    with pytest.raises(ValueError, match="turn_angle"):
        plan_round.plan_best_object_path(obj_slam, slam, _FakePlanner(lengths), agent, 1, 0, dict(forward_step_size=0.25), "fisher")


def test_plan_best_object_path_popgs_goes_to_the_batched_evaluation(monkeypatch):
    from fisher_rast import path_eval, plan_round
    lengths = [4, 9, 0, 2, 7] + [5 + k for k in range(20)]
    obj_slam = types.SimpleNamespace(gaussian_points="object", pose_eval="pose_eval", pose_eval_popgs="pose_eval_popgs", compute_H_train_popgs=lambda: "H_popgs")
    slam = types.SimpleNamespace(gaussian_points="scene")
    seen = {}

    def fake_eval(slam_, start, path_actions, finals, H_train, **kw):
        seen.update(slam=slam_, n=len(path_actions), finals=list(finals), H=H_train, kw=kw)
        return [-10.0 - 0.5 * abs(i - 6) for i in range(len(path_actions))]                  # all below -1: the floor here is -inf
    monkeypatch.setattr(path_eval, "evaluate_paths_popgs", fake_eval)
    pl = _FakePlanner(lengths)
    cfg = dict(forward_step_size=0.25, turn_angle=30., object_path_end_weight=0.3, path_end_weight=1.0, acc_H_train_every=4, lam=1e-5, unknown=1)
    res = plan_round.plan_best_object_path(obj_slam, slam, pl, np.eye(4), 1, 0, cfg, "topt")
    assert pl.calls[0][1:] == ("pose_eval_popgs", "object", "scene", None, 1, False, "topt")
    assert seen["slam"] is obj_slam and seen["n"] == 21 and seen["H"] == "H_popgs" and seen["finals"] == [float(e) for e in res[6][:21]]
    kw = seen["kw"]
    assert kw["criterion"] == "topt" and kw["object_path_end_weight"] == 0.3 and kw["path_end_weight"] == 1.0 and kw["acc_H_train_every"] == 4 and kw["lam"] == 1e-5
    assert "unknown" not in kw and tuple(kw["poses_w2c"].shape) == (21, 200, 4, 4)
    assert res.best_index == 6 and res[0] == res.plan.path_actions[6]
    # a prior the caller holds is used as it is
    res = plan_round.plan_best_object_path(obj_slam, slam, _FakePlanner(lengths), np.eye(4), 1, 0, cfg, "dopt", H_train="mine")
    assert seen["H"] == "mine" and seen["kw"]["criterion"] == "dopt"


def test_fisher_object_path_value():
    from fisher_rast import plan_round
    assert plan_round.fisher_object_path_value(3.0, 4, 0.0) == 0.75 and plan_round.fisher_object_path_value(torch.tensor(3.0), 4, 0.5) == 1.5
    assert "Not rebuilt: action_planning_object (superseded" in plan_round.__doc__ and "action_planning_object_adv / _object" not in plan_round.__doc__


# ---- signatures -----------------------------------------------------------------------------------------------------------------------------

ROOT = gc.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "reference_signatures_goal.json")


def _signature(fn):
    a = fn.args
    pos = [x.arg for x in a.posonlyargs + a.args]
    if pos and pos[0] in ("self", "cls"):
        pos = pos[1:]
    defaults = []
    for d in a.defaults:
        try:
            defaults.append(ast.literal_eval(d))
        except ValueError:
            defaults.append("<expr>")
    return pos, defaults


def test_goal_grafts_accept_the_reference_call_forms():
    with open(FIXTURE) as f:
        ref = json.load(f)
    assert set(ref) == {"AstarPlanner", "NavTester"} and ref["AstarPlanner"]["file"] == "planning/astar.py"
    # names and defaults only: no source text in the fixture
    assert all(set(m) == {"pos", "defaults", "kwonly", "vararg", "kwarg"} for c in ref.values() for m in c["methods"].values())
    tree = ast.parse(open(os.path.join(ROOT, "fisher-nerf-customized_amd", "planning", "astar.py")).read())
    mixin = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == "GoalSelectOps")
    ours = {n.name: n for n in mixin.body if isinstance(n, ast.FunctionDef)}
    install = [e.value for node in ast.walk(ours["install"]) if isinstance(node, ast.For) and isinstance(node.iter, ast.Tuple) for e in node.iter.elts]
    checked = 0
    for name, r in ref["AstarPlanner"]["methods"].items():
        assert name in install and name in ours, name
        pos, defaults = _signature(ours[name])
        assert pos[:len(r["pos"])] == r["pos"], (name, pos, r["pos"])
        # the reference's defaults, value for value; what is added behind is optional
        n_req = len(r["pos"]) - len(r["defaults"])
        assert len(pos) - len(defaults) == n_req, name
        assert defaults[:len(r["defaults"])] == r["defaults"], (name, defaults, r["defaults"])
        checked += 1
    assert checked == 4
    # action_planning_object_adv of plan_round: the planner first, then the reference's parameters
    tree = ast.parse(open(os.path.join(ROOT, "fisher-nerf-customized_amd", "fisher_rast", "plan_round.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "action_planning_object_adv")
    pos, defaults = _signature(fn)
    r = ref["NavTester"]["methods"]["action_planning_object_adv"]
    assert pos[0] == "planner" and pos[1:1 + len(r["pos"])] == r["pos"] and len(pos) - len(defaults) == 1 + len(r["pos"])
