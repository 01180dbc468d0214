"""The object round on the CPU: the follower's arithmetic (csrc/fr_action_object_math.h, compiled with g++ in
tests/harness/fr_goal_harness.cpp) against the NumPy restatement of NavTester.action_planning_object_adv in tests/goal_cases.py on every
case family -- action lists, counts, keep flags, pruned paths and cells exactly, positions to 1e-12, the binary32 inverses to one ulp of
float32(np.linalg.inv) -- each case's decision margins asserted first and the defensive bound never reached; the object cells and the
grid's tables against their NumPy restatements; the stand-alone harness program under the address and undefined-behaviour sanitizers;
the ABI's rejections, which need no device."""
import ctypes
import os

import numpy as np
import pytest

import goal_cases as gc
import harness_build


@pytest.fixture(scope="module")
def harness():
    return gc.build_harness()


_CACHE = {}


def _computed(h, family):
    """the case, what the harness makes of it and what the restatement does -- once per family"""
    if family not in _CACHE:
        c = gc.make_case(family)
        _CACHE[family] = (c, gc.harness_plan(h, c), gc.np_action_planning_object_adv(c))
    return _CACHE[family]


@pytest.mark.parametrize("family", gc.FAMILIES)
def test_harness_equals_the_restatement(harness, family):
    c, got, want = _computed(harness, family)
    assert want["margin"] > gc.MARGIN and want["yaw_margin"] > gc.YAW_MARGIN, (family, want["margin"], want["yaw_margin"])
    worst_xz, worst_ulp = gc.compare(got, want, c)
    print(f"{family}: margin {want['margin']:.3g}  yaw margin {want['yaw_margin']:.3g}  c2w_xz {worst_xz:.3g}  w2c ulps {worst_ulp}  "
          f"longest free run {want['free_run']}")
    assert got["n_actions"].max() <= gc.Q == harness.frg_h_object_max()
    # the defensive bound on free stage advances is never reached, in the harness or in the restatement
    assert not got["bound_hit"].any()
    assert want["free_run"] <= max(int(n) for n in c["lengths"]) + 1


def test_the_families_sit_on_their_decisions(harness):
    # G = 1
    c, got, want = _computed(harness, "g1")
    assert want["keep"] == [1] and 1 in want["actions"][0]
    # paths of 2, 63, 64, 65 and 130 points: survivors on both sides of a lane and a chunk boundary, and some pruned
    c, got, want = _computed(harness, "lanes")
    assert c["lengths"].tolist() == [2, 63, 64, 65, 130, 100]
    for g in (1, 2, 3, 4, 5):
        assert 2 <= len(want["pruned"][g]) < c["lengths"][g], (g, len(want["pruned"][g]))
    assert len(want["pruned"][4]) > 64                                  # the chunk base is carried
    xs = want["pruned"][5][:, 0] - c["start"][0]                        # the path that runs past the goal: a gap across the 64th point
    assert xs.min() == 0 and xs.max() == 99 and not ((xs > 60) & (xs < 68)).any() and (xs < 60).any() and (xs > 68).any()
    # a path of one point: `finish` = (row, col) goes into the x-z list as it is; the same point again when it equals the finish
    c, got, want = _computed(harness, "one-point")
    assert c["lengths"].tolist() == [1, 1, 1] and c["start"][0] != c["start"][1]
    assert want["pruned"][0].tolist()[-1] == c["goals"][0].tolist() != [c["goals"][0][1], c["goals"][0][0]]
    # every waypoint pruned: [first, last] is left
    c, got, want = _computed(harness, "all-pruned")
    for g in (0, 1):
        assert want["pruned"][g].tolist() == [c["paths"][g, 0].tolist(), c["paths"][g, c["lengths"][g] - 1].tolist()]
    # reached in position at the start: orientation-only from step 0, in both directions; within one turn: an empty list, which is dropped
    c, got, want = _computed(harness, "at-goal")
    assert set(want["actions"][0]) == {2} and set(want["actions"][1]) == {3}
    assert want["orientation_only"][0] == want["n_actions"][0] >= 2 and want["orientation_only"][1] == want["n_actions"][1] >= 2
    assert want["n_actions"][2:] == [0, 0] and want["keep"] == [1, 1, 0, 0]
    # the jump to the goal, and waypoints taken one by one
    c, got, want = _computed(harness, "skip")
    # (the last waypoint lies at the goal, so the step onto it always counts as a jump)
    assert want["skipped"][0] == 1 and want["advanced"][0] == 0 and want["advanced"][1] >= 2
    # the cap
    c, got, want = _computed(harness, "cap")
    assert want["n_actions"][0] == 200 and 0 < want["n_actions"][1] < 200
    # an odd grid with its centre off the origin; lengths 0 and -1 mixed in
    c, got, want = _computed(harness, "odd-grid")
    assert c["W"] % 2 == 1 and c["H"] % 2 == 1 and c["center"] != (0.0, 0.0)
    assert want["n_actions"][2] == want["n_actions"][6] == -1 and sorted(c["lengths"][[2, 6]]) == [-1, 0]
    # more goals than a wave has lanes, with a duplicate beyond the 64th
    c, got, want = _computed(harness, "g70")
    assert len(want["keep"]) == 70 and want["keep"][69] == 0 and want["n_actions"][69] > 0 and want["keep"][40] == 0 and sum(want["keep"]) > 20
    c, got, want = _computed(harness, "all-without-path")
    assert want["n_actions"] == [-1, -1, -1] and want["keep"] == [0, 0, 0] and not got["pruned"].any()


def test_one_point_left_after_pruning_gets_the_finish(harness):
    """a two-point path whose end lies at the goal and whose start does not: the end is pruned, one point is left, `finish` is appended"""
    c, got, want = _computed(harness, "one-left")
    sx, sz = c["start"]
    for g in (0, 1):
        assert c["lengths"][g] == 2 and want["pruned"][g].tolist() == [[sx, sz], [sz, sx + 12]]          # the survivor, then (row, col) as it is
        assert got["pruned_len"][g] == 2 and got["pruned"][g, :2].tolist() == [[sx, sz], [sz, sx + 12]]


def test_the_height_quirk_changes_which_waypoints_survive(harness):
    c, got, want = _computed(harness, "height-quirk")
    assert c["agent"][1, 3] != c["cam_height"]
    fixed = gc.np_action_planning_object_adv(c, fixed_prune=True)
    for g in (0, 1):
        assert len(fixed["pruned"][g]) < len(want["pruned"][g]), "the fixed formula prunes the waypoints near the goal, the reference's does not"
    assert fixed["actions"] != want["actions"]
    # and the harness follows the reference, not the fixed formula
    assert [p.tolist() for p in want["pruned"]] == [got["pruned"][g, :got["pruned_len"][g]].tolist() for g in range(2)]


def test_object_cells_harness_equals_np_unique(harness):
    rng = np.random.default_rng(3)
    for (W, H, cell, center) in ((67, 71, 0.05, (0.37, -1.21)), (128, 128, 0.05, (0.0, 0.0))):
        pol = gc.Policy(dict(W=W, H=H, cell=cell, center=center, cam_height=0.4))
        for n in (0, 1, 300, 5000):
            pts = np.zeros((n, 3), np.float32)
            if n:
                spots = rng.uniform(-0.9, 0.9, (12, 2)) * np.array([W, H]) * cell / 2 + np.asarray(center)
                pts[:, [0, 2]] = spots[rng.integers(0, 12, n)] + rng.uniform(-0.04, 0.04, (n, 2))
            if n >= 300:
                pts[:7, [0, 2]] = pol.world_at(np.array([5.5, 9.5])) + 0.3 * cell                     # seven in one place near a corner
                pts[7:10, [0, 2]] = [50.0, 50.0]                                                       # outside: the border cell
                pts[10:14, [0, 2]] = [-50.0, 1e30]
                pts[14] = [np.nan, 0, 0]
                pts[15] = [0, 0, np.inf]
            for max_cells in (W * H, 2):
                cells = np.full((max_cells, 2), 0x5A5A5A5A, np.int32)
                counts = np.zeros(2, np.int32)
                p = np.ascontiguousarray(pts)
                harness.frg_h_object_cells(W, H, cell, center[0], center[1], p.ctypes.data, n, 3, cells.ctypes.data, max_cells, counts.ctypes.data)
                want_cells, want_counts = gc.np_object_cells(W, H, cell, center, pts, 3, max_cells)
                assert counts.tolist() == want_counts, (W, n, max_cells)
                assert np.array_equal(cells[:len(want_cells)], want_cells) and (cells[len(want_cells):] == 0x5A5A5A5A).all()
                if n >= 300 and max_cells == W * H:
                    # two rows are not finite; the border cell with exactly 3 is left out, the one with exactly 4 is in
                    assert want_counts[1] == n - 2 and [W - 1, H - 1] not in want_cells.tolist() and [0, H - 1] in want_cells.tolist()


def test_grid_tables_equal_the_linspaces(harness):
    assert gc.n_theta_of(15.0) == 24 and gc.n_theta_of(360.0) == 1 and gc.n_theta_of(180.0) == 2 and gc.n_theta_of(1000.0) == 1
    for n_theta in (1, 2, 3, 24, 360):
        for bins in (1, 2, 6):
            for sqrt_area in (0, 1):
                angles = np.full(max(1, n_theta - 1), np.nan, np.float32)
                radii = np.full(bins, np.nan, np.float32)
                harness.frg_h_tables(n_theta, bins, sqrt_area, 0.2, 1.7, angles.ctypes.data, radii.ctypes.data)
                want_a, want_r = gc.np_grid_tables(n_theta, bins, sqrt_area, 0.2, 1.7)
                assert np.array_equal(angles, want_a) and np.array_equal(radii, want_r), (n_theta, bins, sqrt_area)
    a, _ = gc.np_grid_tables(24, 6, 0, 0.2, 1.7)
    assert len(a) == 23                                                            # the reference drops the closing angle: 23, not 24


def test_grid_poses_of_the_harness_equal_the_restatement(harness):
    centers = np.array([[0.3, -0.2], [1.1, 0.4], [-0.7, 0.9]], np.float32)
    for K in (1, 33, 138, 139, 300):
        for bins, sqrt_area in ((1, 0), (6, 0), (6, 1)):
            for n_theta in (1, 24):
                c2w = np.full((K, 4, 4), np.nan, np.float32)
                harness.frg_h_grid(centers.ctypes.data, 3, K, 0.2, 1.5, n_theta, bins, sqrt_area, 0.4, 123, c2w.ctypes.data)
                want, _ = gc.np_grid_candidates(96, 96, 0.05, (0.0, 0.0), centers, K, 0.2, 1.5, n_theta, bins, sqrt_area, 0.4, 123)
                assert np.abs(c2w - want).max() <= 2e-6, (K, bins, sqrt_area, n_theta)


def test_harness_program_under_sanitizers(tmp_path):
    """the stand-alone program (its own main) over the same headers, under -fsanitize=address,undefined"""
    r = harness_build.sanitized_program("fr_goal_harness", "FRG_HARNESS_MAIN", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checksum" in r.stdout and not r.stderr.strip()


def test_sources_exports_and_header(harness):
    from fisher_rast import _lib
    for n in ("fr_goal.hip", "fr_action_object.hip", "fr_goal_math.h", "fr_action_object_math.h"):
        assert os.path.join(_lib._CSRC, n) in (_lib.UNITS if n.endswith(".hip") else _lib.SOURCES), n
    header = open(os.path.join(gc.ROOT, "include", "fisher_occ.h")).read()
    for name in ("fr_plan_actions_object", "fr_occ_object_cells", "fr_occ_grid_candidates"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define FR_ACTION_OBJECT_MAX {_lib.FR_ACTION_OBJECT_MAX}" in header and _lib.FR_ACTION_OBJECT_MAX == harness.frg_h_object_max() == 200
    assert "#define FR_ACTION_MAX_QUEUE 128" in header                              # the planning queue's cap is not raised
    for unit in ("fr_goal.hip", "fr_action_object.hip"):
        src = open(os.path.join(gc.ROOT, "fisher-nerf-customized_amd", "csrc", unit)).read()
        assert "hipMalloc" not in src and "hipMemcpy" not in src and "Synchronize" not in src and "getenv" not in src


def test_abi_rejections_need_no_device():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    lib = _lib.load()
    ok = _lib.OccCfg(70, 67, 0.05, 0.0, 0.0, -0.6, 0.6, 10.0)
    A = 1 << 20                                   # addresses that are never dereferenced: every call below is refused on the host
    eye = (ctypes.c_double * 16)(*np.eye(4).reshape(-1))
    nan = (ctypes.c_double * 16)(*([float("nan")] + [0.0] * 15))
    big = lib.fr_occ_workspace_bytes(ctypes.byref(ok))

    def plan(cfg=ok, paths=A, max_len=8, lengths=A, goals=A, poses=A, G=2, agent=eye, h=0.4, step=0.065, turn=10., cell=0.05, actions=A, n=A,
             keep=A, w2c=A, xz=A, cells=A, pruned=A, plen=A):
        return lib.fr_plan_actions_object(ctypes.byref(cfg) if cfg else None, paths, max_len, lengths, goals, poses, G, agent, h, step, turn, cell,
                                          actions, n, keep, w2c, xz, cells, pruned, plen, None)

    def cells(cfg=ok, points=A, n=5, min_count=3, out=A, max_cells=9, counts=A, ws=A, ws_bytes=big):
        return lib.fr_occ_object_cells(ctypes.byref(cfg) if cfg else None, points, n, min_count, out, max_cells, counts, ws, ws_bytes, None)

    def grid(cfg=ok, centers=A, n_centers=3, cell_list=None, n_dev=None, K=8, lo=0.2, hi=1.5, n_theta=24, bins=6, sqrt_area=0, h=0.4, seed=1,
             eroded=None, min_free=40, c2w=A, keep=A):
        return lib.fr_occ_grid_candidates(ctypes.byref(cfg) if cfg else None, centers, n_centers, cell_list, n_dev, K, lo, hi, n_theta, bins, sqrt_area,
                                          h, seed, eroded, min_free, c2w, keep, None)

    bad_cfg = _lib.OccCfg(0, 67, 0.05, 0, 0, 0, 0, 0)
    bad_cell = _lib.OccCfg(70, 67, 0.0, 0, 0, 0, 0, 0)
    for call, name, bads in (
            (plan, b"fr_plan_actions_object",
             [dict(cfg=None), dict(cfg=bad_cfg), dict(paths=None), dict(lengths=None), dict(goals=None), dict(poses=None), dict(actions=None), dict(n=None),
              dict(keep=None), dict(w2c=None), dict(xz=None), dict(cells=None), dict(pruned=None), dict(plen=None), dict(agent=None), dict(agent=nan),
              dict(G=-1), dict(max_len=0), dict(step=0.0), dict(step=float("inf")), dict(turn=0.0), dict(turn=float("nan")), dict(cell=0.0),
              dict(cell=float("inf")), dict(h=float("nan")), dict(paths=A + 2), dict(lengths=A + 1), dict(xz=A + 4), dict(n=A + 3), dict(w2c=A + 2),
              dict(pruned=A + 1), dict(plen=A + 2)]),
            (cells, b"fr_occ_object_cells",
             [dict(cfg=None), dict(cfg=bad_cfg), dict(cfg=bad_cell), dict(points=None), dict(out=None), dict(counts=None), dict(ws=None), dict(n=-1),
              dict(min_count=-1), dict(max_cells=-1), dict(points=A + 2), dict(out=A + 1), dict(counts=A + 3), dict(ws=A + 8)]),
            (grid, b"fr_occ_grid_candidates",
             [dict(cfg=None), dict(cfg=bad_cfg), dict(cfg=bad_cell), dict(K=-1), dict(n_centers=-1), dict(n_centers=0), dict(centers=None),
              dict(cell_list=A), dict(centers=None, cell_list=A), dict(c2w=None), dict(n_theta=0), dict(bins=0), dict(bins=1 << 16, n_theta=1 << 16),
              dict(lo=float("nan")), dict(hi=float("inf")), dict(lo=-0.1), dict(h=float("nan")), dict(centers=A + 2), dict(c2w=A + 1),
              dict(centers=None, cell_list=A + 2, n_dev=A), dict(centers=None, cell_list=A, n_dev=A + 2)])):
        for bad in bads:
            assert call(**bad) == _lib.FR_EINVAL, (name, bad)
            assert name in lib.fr_last_error(), (name, bad)
    assert cells(ws_bytes=big - 1) == _lib.FR_ENOSPACE and b"fr_occ_object_cells" in lib.fr_last_error()
    # nothing to do: no launch, whatever the pointers (a launch would fail here, there is no device)
    assert plan(G=0, paths=None, lengths=None, goals=None, poses=None, actions=None, n=None, keep=None, w2c=None, xz=None, cells=None, pruned=None,
                plen=None) == _lib.FR_OK
    assert grid(K=0, centers=None, c2w=None, keep=None) == _lib.FR_OK
    # but the arguments are still checked with nothing to do
    assert plan(G=0, step=0.0) == _lib.FR_EINVAL and grid(K=0, n_theta=0) == _lib.FR_EINVAL
