"""The path planner on the CPU: the cost model (csrc/fr_plan_math.h, compiled with g++ in tests/harness/fr_plan_harness.cpp, with a plain
Dijkstra driver) against the NumPy / heapq restatements of tests/plan_cases.py on every map family -- the grid, the tier bytes, the
packed field word for word, the paths; the dominance over the reference-order best-first search; the paths' own properties; the
stand-alone harness program under the address and undefined-behaviour sanitizers; the ABI's rejections, which need no device; the
install on a stand-in class.  There is no reference-run fixture for this stage: the reference's planning needs cv2."""
import ctypes
import os
import sys
import types

import numpy as np
import pytest

import harness_build
import plan_cases as pc


@pytest.fixture(scope="module")
def plan_harness():
    return pc.build_harness()


_CACHE = {}


def _computed(h, family):
    """the case, what the harness makes of it and what the restatement does -- once per family"""
    if family not in _CACHE:
        c = pc.make_case(family)
        got = {s: pc.harness_plan(h, c, shortcut=s) for s in (False, True)}
        occ_plan, status = pc.np_grid(c)
        field = pc.np_field(c["free"], c["start"])
        want = dict(occ_plan=occ_plan, status=status, tiers=pc.np_tiers(c["free"]), field=field,
                    paths={s: pc.np_paths(field, occ_plan, c["start"], c["goals"], s) for s in (False, True)})
        _CACHE[family] = (c, got, want)
    return _CACHE[family]


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_harness_equals_the_restatement(plan_harness, family):
    c, got, want = _computed(plan_harness, family)
    g = got[True]
    assert np.array_equal(g["occ_plan"], want["occ_plan"])
    assert g["status"].tolist() == want["status"].tolist()
    assert np.array_equal(g["tiers"], want["tiers"])
    assert g["in_free"] == int(c["free"][c["start"]] != 0)
    assert np.array_equal(g["field"], want["field"]), "the field differs (cost bits or parent)"
    for s in (False, True):
        assert len(got[s]["paths"]) == len(c["goals"])
        for goal, a, b in zip(c["goals"], got[s]["paths"], want["paths"][s]):
            assert np.array_equal(a.reshape(-1, 2), b.reshape(-1, 2)), (family, s, goal)


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_paths_are_table_moves_over_free_corridors_and_sum_to_the_field(plan_harness, family):
    c, got, _ = _computed(plan_harness, family)
    weights = pc.move_weights(c["free"])
    cost = pc.field_cost(got[False]["field"])
    some = 0
    for path in got[False]["paths"]:
        if len(path) == 0:
            continue
        some += 1
        cells = [(int(z), int(x)) for x, z in path]
        assert cells[0] == c["start"] and len(cells) >= 2
        total = pc.path_cost32(c["free"], cells, weights)                    # raises on a step that is no free table move
        assert np.float32(total).view(np.uint32) == np.float32(cost[cells[-1]]).view(np.uint32)
    if family == "start-outside-free":
        assert some == 0
    else:
        assert some > 0, "no goal of this family has a path"
    # the shortcut keeps the ends, and only ever drops points
    for a, b in zip(got[False]["paths"], got[True]["paths"]):
        assert (len(a) == 0) == (len(b) == 0)
        if len(a):
            assert a[0].tolist() == b[0].tolist() and a[-1].tolist() == b[-1].tolist() and len(b) <= max(len(a), 3)
            assert {tuple(p) for p in b.tolist()} <= {tuple(p) for p in a.tolist()}


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_field_is_never_above_the_reference_order_search(plan_harness, family):
    """where the best-first search of the reference reaches a cell, its path there, summed in binary32, costs at least the field's value.
    The start itself is left out: the search holds it from the beginning, in free space or not, and returns no path to it."""
    c, got, _ = _computed(plan_harness, family)
    cost = pc.field_cost(got[False]["field"])
    weights = pc.move_weights(c["free"])
    bf = pc.BestFirst(got[False]["occ_plan"], c["free"], c["start"])
    checked = 0
    for goal in c["goals"]:
        path = bf.planning(goal)
        if path:
            assert cost[path[-1]] >= 0 and pc.path_cost32(c["free"], path, weights) >= cost[path[-1]], (family, goal)
        for cell, total in bf.tree_costs32(weights).items():
            if cell != c["start"]:
                assert 0 <= cost[cell] <= total, (family, goal, cell)
                checked += 1
    assert checked > 0 or family == "start-outside-free"


def test_the_families_sit_on_their_decisions(plan_harness):
    h = plan_harness
    # the tiers switch between L1 distances 5 | 6, 10 | 11, 20 | 21 of the one obstacle
    c, got, _ = _computed(h, "tier-thresholds")
    t = got[True]["tiers"]
    assert [int(t[y, x]) >> 1 for y, x in [(25, 15), (25, 16), (25, 20), (25, 21), (25, 30), (25, 31), (22, 12), (21, 12)]] == [3, 2, 2, 1, 1, 0, 3, 2]
    assert t[25, 10] == 0 and t[0, 63] == 1                       # the obstacle is not free; the map's border is no obstacle
    # 51 Gaussians in the band occupy a cell (and its dilation), 50 do not, nor do 51 outside the band or outside the grid
    c, got, _ = _computed(h, "gaussians")
    occ = got[True]["occ_plan"]
    assert occ[9:12, 9:12].all() and occ[44:46, 0:2].all() and occ[0:2, 50:52].all() and int(occ.sum()) == 9 + 4 + 4
    assert got[True]["status"][1] == 51 + 50 + 26 + 51 + 51
    assert len(got[True]["paths"][0]) == 0 and len(got[True]["paths"][1]) == 0 and len(got[True]["paths"][2]) > 0
    assert not pc.harness_grid(h, c, points=None)[0].any()
    # a ring of 7 leaves the start alone, a ring of 8 is what the Python layer raises on
    assert _computed(h, "ring-7")[1][True]["status"][0] == 7 and _computed(h, "ring-8")[1][True]["status"][0] == 8
    # the widening goes by table index: the eastward move (row 4) is widened along x, its own direction, and stays one cell wide --
    # it passes a door of one cell, as in the reference
    for fam in ("door-1", "door-3", "door-9"):
        assert len(_computed(h, fam)[1][True]["paths"][0]) > 0
    assert pc.move_weights(_computed(h, "door-1")[0]["free"])[0][4, 20, 22]
    # the island and the start outside the free space
    c, got, _ = _computed(h, "island")
    assert len(got[True]["paths"][0]) == 0 and (pc.field_cost(got[True]["field"])[11:29, 31:48] < 0).all()
    c, got, _ = _computed(h, "start-outside-free")
    assert got[True]["in_free"] == 0 and (got[True]["field"] == pc.UNREACHED).all() and not any(len(p) for p in got[True]["paths"])
    # two routes: the straight way through the corridor is shorter, the way round the slab is cheaper
    c, got, _ = _computed(h, "two-routes")
    path = got[False]["paths"][0]
    assert len(path) and not any(20 <= z < 80 and 40 <= x <= 60 for x, z in path.tolist())
    # a two-point path gets its last point twice from the shortcut loop, as in the reference
    c, got, _ = _computed(h, "empty-room")
    two = [(a, b) for a, b in zip(got[False]["paths"], got[True]["paths"]) if len(a) == 2]
    assert two and all(len(b) == 3 and b[1].tolist() == b[2].tolist() for _, b in two)
    # the serpentine's far goal is reached over many lanes, and the shortcut shortens the list
    c, got, _ = _computed(h, "serpentine")
    assert len(got[False]["paths"][0]) > 30 and len(got[True]["paths"][0]) < len(got[False]["paths"][0])


def test_max_len_one_short_gives_minus_one(plan_harness):
    """the path as walked has to fit, shortcut or not: it is shortcut in place"""
    c, got, _ = _computed(plan_harness, "serpentine")
    n = len(got[False]["paths"][0])
    for s in (False, True):
        paths, lengths = pc.harness_paths(plan_harness, got[s]["field"], got[s]["occ_plan"], c["start"], c["goals"][:1], s, max_len=n - 1)
        assert lengths.tolist() == [-1]
        paths, lengths = pc.harness_paths(plan_harness, got[s]["field"], got[s]["occ_plan"], c["start"], c["goals"][:1], s, max_len=n)
        assert lengths.tolist() == [len(got[s]["paths"][0])] and np.array_equal(paths[0, :lengths[0]], got[s]["paths"][0])
    # a two-point path needs room for three under the shortcut
    c, got, _ = _computed(plan_harness, "empty-room")
    k = [len(p) for p in got[False]["paths"]].index(2)
    for s, room, want in ((False, 2, 2), (True, 2, -1), (True, 3, 3)):
        assert pc.harness_paths(plan_harness, got[s]["field"], got[s]["occ_plan"], c["start"], c["goals"][k:k + 1], s, max_len=room)[1].tolist() == [want]


def test_harness_program_under_sanitizers(tmp_path):
    """the stand-alone program (its own main) over the same header, under -fsanitize=address,undefined"""
    r = harness_build.sanitized_program("fr_plan_harness", "FRP_HARNESS_MAIN", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checksum" in r.stdout and not r.stderr.strip()


def test_install_on_a_stand_in_class():
    from planning import astar
    mod = types.ModuleType("fake_ref_astar")
    sys.modules[mod.__name__] = mod
    try:
        keep = lambda self: None
        cls = type("RefPlanner", (), {"__module__": mod.__name__, "setup_start": keep, "planning": keep, "CheckCollision": keep, "other": keep})
        assert astar.PathPlanOps.install(cls) is cls
        for name in ("setup_start", "planning", "plan_paths", "plan_field"):
            assert getattr(cls, name) is astar.PathPlanOps.__dict__[name]
        assert cls.other is keep and cls.CheckCollision is keep
        assert issubclass(mod.LocalizationError, Exception) and astar.PathPlanOps._localization_error(cls) is mod.LocalizationError
        # a module that has the class keeps its own
        own = type("LocalizationError", (RuntimeError,), {})
        mod.LocalizationError = own
        astar.PathPlanOps.install(cls)
        assert mod.LocalizationError is own
    finally:
        del sys.modules[mod.__name__]
    # opt-in: the occupancy mixin does not carry the planner; the product's own class does
    assert not hasattr(astar.OccupancyOps, "planning") and issubclass(astar.AstarPlanner, astar.PathPlanOps)


def test_abi_rejections_need_no_device():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    lib = _lib.load()
    ok = _lib.OccCfg(70, 67, 0.05, 0.0, 0.0, -0.6, 0.6, 10.0)
    bad_cfgs = [_lib.OccCfg(0, 67, 0.05, 0, 0, 0, 0, 0), _lib.OccCfg(70, -1, 0.05, 0, 0, 0, 0, 0), _lib.OccCfg(70, 67, 0.0, 0, 0, 0, 0, 0),
                _lib.OccCfg(1 << 16, 1 << 15, 0.05, 0, 0, 0, 0, 0)]
    need = int(lib.fr_plan_workspace_bytes(ctypes.byref(ok)))
    assert need >= 70 * 67 * (16 + 4 + 1) and lib.fr_plan_workspace_bytes(None) == 0
    assert lib.fr_plan_round_cap(ctypes.byref(ok)) >= 4 * 4 and lib.fr_plan_round_cap(None) == 0
    for b in bad_cfgs:
        assert lib.fr_plan_workspace_bytes(ctypes.byref(b)) == 0 and lib.fr_plan_round_cap(ctypes.byref(b)) == 0
    # addresses that are never dereferenced: every call below is refused on the host
    A, big = 1 << 20, 1 << 40
    E = (_lib.FR_EINVAL, _lib.FR_ENOSPACE)

    def grid(cfg=ok, occ=A, pts=None, n=0, sy=3, sx=4, out=A, status=A, ws=A, nws=big):
        return lib.fr_plan_grid(ctypes.byref(cfg) if cfg else None, occ, pts, n, 0.5, sy, sx, out, status, ws, nws, None)

    def tiers(cfg=ok, free=A, out=A):
        return lib.fr_plan_tiers(ctypes.byref(cfg) if cfg else None, free, out, None)

    def field(cfg=ok, t=A, sy=3, sx=4, f=A, status=A, ws=A, nws=big):
        return lib.fr_plan_field(ctypes.byref(cfg) if cfg else None, t, sy, sx, f, status, None, ws, nws, None)

    def paths(cfg=ok, f=A, occ=A, sy=3, sx=4, goals=A, G=2, paths=A, max_len=8, lengths=A):
        return lib.fr_plan_paths(ctypes.byref(cfg) if cfg else None, f, occ, sy, sx, goals, G, 1, paths, max_len, lengths, None)

    for call, name, bads in (
            (grid, b"fr_plan_grid", [dict(cfg=None), dict(occ=None), dict(out=None), dict(status=None), dict(n=-1), dict(sy=-1), dict(sy=67), dict(sx=70),
                                     dict(ws=None), dict(nws=need - 1), dict(ws=A + 8), dict(occ=A + 2), dict(pts=A + 1, n=3), dict(status=A + 2)]),
            (tiers, b"fr_plan_tiers", [dict(cfg=None), dict(free=None), dict(out=None)]),
            (field, b"fr_plan_field", [dict(cfg=None), dict(t=None), dict(f=None), dict(status=None), dict(sy=67), dict(sx=-1), dict(f=A + 4),
                                       dict(status=A + 1), dict(ws=None), dict(nws=need - 1), dict(ws=A + 4)]),
            (paths, b"fr_plan_paths", [dict(cfg=None), dict(f=None), dict(occ=None), dict(goals=None), dict(lengths=None), dict(paths=None), dict(G=-1),
                                       dict(max_len=-1), dict(sy=67), dict(f=A + 4), dict(goals=A + 2), dict(paths=A + 1), dict(lengths=A + 3)])):
        for bad in bads:
            assert call(**bad) in E, (name, bad)
            assert name in lib.fr_last_error(), (name, bad)
        for b in bad_cfgs:
            assert call(cfg=b) == _lib.FR_EINVAL, name
    # no goals: nothing to launch, whatever the pointers
    assert paths(G=0, f=None, occ=None, goals=None, paths=None, lengths=None) == _lib.FR_OK
