"""-m gpu: the path planner (fr_plan_grid / fr_plan_tiers / fr_plan_field / fr_plan_paths, csrc/fr_plan.hip) and the Python layer on it
(planning/astar.py: PathPlanOps).

Through the C ABI on guarded buffers against the g++ harness over the same header (tests/harness/fr_plan_harness.cpp, a plain
Dijkstra): the planning grid, the tier bytes, the packed field, the paths and their lengths equal, guards intact -- at the smallest
shapes at which the kernels can still go wrong: 8 x 8 (less than a tile, the start in a corner), 70 x 67 (ragged tiles, one tile
border each way), 130 x 130 with the serpentine (3 x 3 tiles, a path that crosses tile borders back and forth: many rounds, below
the cap).  G = 0, 1 and 21; goals occupied, unreachable, next to the start, on the border, outside the grid; max_len one short of a
path; the shortcut on and off; no Gaussians.  Through the Python layer: plan_paths against planning goal by goal and against the
harness on the free space the device built, the host reads counted, LocalizationError on a ringed start."""
import ctypes

import numpy as np
import pytest
import torch

import plan_cases as pc

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes behind every buffer
GUARD_BYTE = 0x5A


@pytest.fixture(scope="module")
def plan_harness():
    return pc.build_harness()


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


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _cfg(c):
    from fisher_rast import _lib
    return _lib.OccCfg(c["W"], c["H"], c["cell"], c["center"][0], c["center"][1], -0.6, 0.6, 10.0)


def _field(dev, c, points="case"):
    """fr_plan_grid, fr_plan_tiers and fr_plan_field on guarded buffers: dict(occ_plan, status, tiers, field, counts, cap, buffers)"""
    from fisher_rast import _lib
    lib = _lib.load()
    H, W = c["H"], c["W"]
    cfg = _cfg(c)
    nws = int(lib.fr_plan_workspace_bytes(ctypes.byref(cfg)))
    assert nws > 0
    b = dict(occ=_Guarded(H * W, dev), tiers=_Guarded(H * W, dev), field=_Guarded(8 * H * W, dev), status=_Guarded(16, dev), ws=_Guarded(nws, dev))
    occ_map, free = _dev(c["occ_map"], dev), _dev(c["free"], dev)
    pts = c["points"] if isinstance(points, str) else points
    pts_d = None if pts is None else _dev(np.asarray(pts, np.float32), dev)
    sy, sx = c["start"]
    _lib.check(lib.fr_plan_grid(ctypes.byref(cfg), occ_map.data_ptr(), None if pts_d is None else pts_d.data_ptr(), 0 if pts is None else len(pts),
                                c["cam_height"], sy, sx, b["occ"].ptr, b["status"].ptr, b["ws"].ptr, nws, _stream(dev)), "fr_plan_grid")
    _lib.check(lib.fr_plan_tiers(ctypes.byref(cfg), free.data_ptr(), b["tiers"].ptr, _stream(dev)), "fr_plan_tiers")
    counts = (ctypes.c_int32 * 2)()
    _lib.check(lib.fr_plan_field(ctypes.byref(cfg), b["tiers"].ptr, sy, sx, b["field"].ptr, b["status"].ptr, ctypes.byref(counts), b["ws"].ptr, nws,
                                 _stream(dev)), "fr_plan_field")
    torch.cuda.synchronize()
    return dict(occ_plan=b["occ"].get(np.uint8).reshape(H, W), tiers=b["tiers"].get(np.uint8).reshape(H, W), status=b["status"].get(np.int32),
                field=b["field"].get(np.uint64).reshape(H, W), counts=(int(counts[0]), int(counts[1])), cap=int(lib.fr_plan_round_cap(ctypes.byref(cfg))),
                buffers=b, intact=all(g.intact() for g in b.values()))


def _paths(dev, c, f, goals, shortcut, max_len=None):
    """fr_plan_paths on the device buffers of `f`: (paths int32 [G, max_len, 2], lengths int32 [G], guards intact)"""
    from fisher_rast import _lib
    lib = _lib.load()
    G = len(goals)
    max_len = c["H"] * c["W"] + 1 if max_len is None else max_len
    paths, lengths = _Guarded(8 * G * max_len, dev), _Guarded(4 * G, dev)
    g = _dev(np.asarray(goals, np.int32).reshape(G, 2), dev) if G else None
    cfg = _cfg(c)
    _lib.check(lib.fr_plan_paths(ctypes.byref(cfg), f["buffers"]["field"].ptr, f["buffers"]["occ"].ptr, c["start"][0], c["start"][1],
                                 None if g is None else g.data_ptr(), G, int(shortcut), paths.ptr, max_len, lengths.ptr, _stream(dev)), "fr_plan_paths")
    torch.cuda.synchronize()
    ok = paths.intact() and lengths.intact() and all(b.intact() for b in f["buffers"].values())
    return paths.get(np.int32).reshape(G, max_len, 2), lengths.get(np.int32), ok


def _small():
    """8 x 8, less than a tile: the start in a corner, one obstacle"""
    label = np.full((8, 8), 2)
    label[5, 5] = 1
    goals = [(5, 5), (4, 4), (0, 1), (7, 0), (0, 7), (7, 7), (3, 0), (9, 3), (-1, 0), (0, 0), (1, 1), (0, 3), (3, 3), (6, 2), (2, 6), (7, 3), (3, 7), (6, 6), (0, 6),
             (6, 0), (1, 4)]
    return pc._case(label, (0, 0), goals)


def _ragged():
    """70 x 67: walls across both tile borders, an island the start cannot reach, Gaussian columns of 50 and 51"""
    H, W = 70, 67
    label = np.full((H, W), 2)
    label[20, :50] = 1
    label[40:, 30] = 1
    label[48:60, 45] = label[48:60, 58] = 1
    label[48, 45:59] = label[59, 45:59] = 1
    pts = [pc.point_at(10, 62, W, H)] * 51 + [pc.point_at(20, 62, W, H)] * 50 + [pc.point_at(66, 69, W, H, y=0.6)] * 51 + [[9.0, 0.2, 0.0]] * 60
    extra = [(52, 50), (62, 10), (20, 10), (21, 10), (66, 3), (69, 66), (0, 66), (4, 3), (3, 6), (69, 29)]
    return pc._case(label, (3, 3), pc._goals(label, (3, 3), extra=extra), points=np.array(pts, np.float32))


CASES = {"8x8": _small, "70x67": _ragged, "130x130-serpentine": lambda: pc.serpentine(130, 130)}
_DONE = {}


def _planned(dev, h, name):
    """the case, the harness's answer and the device's, once per shape"""
    if name not in _DONE:
        c = CASES[name]()
        _DONE[name] = (c, {s: pc.harness_plan(h, c, shortcut=s) for s in (False, True)}, _field(dev, c))
    return _DONE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_field_equals_the_harness(gpu, plan_harness, name):
    c, want, got = _planned(gpu, plan_harness, name)
    w = want[True]
    assert got["intact"]
    assert np.array_equal(got["occ_plan"], w["occ_plan"])
    assert np.array_equal(got["tiers"], w["tiers"])
    rounds, launched, reads = int(got["status"][3]), *got["counts"]
    print(f"{name}: rounds {rounds} launched {launched} reads {reads} cap {got['cap']}")
    assert got["status"][:3].tolist() == [int(w["status"][0]), int(w["status"][1]), w["in_free"]]
    assert np.array_equal(got["field"], w["field"]), "the field differs (cost bits or parent)"
    assert 0 < rounds < launched <= got["cap"] and reads >= 1
    if name == "130x130-serpentine":
        assert rounds > 9, "the serpentine is meant to need more rounds than it has tiles"
    if name == "70x67":
        assert w["status"][1] == 101 and w["occ_plan"][61:64, 9:12].all() and not w["occ_plan"][62, 20]


@pytest.mark.parametrize("name", list(CASES))
def test_paths_equal_the_harness(gpu, plan_harness, name):
    c, want, got = _planned(gpu, plan_harness, name)
    assert len(c["goals"]) == 21
    for shortcut in (False, True):
        w = want[shortcut]
        for G in (0, 1, 21):
            paths, lengths, ok = _paths(gpu, c, got, c["goals"][:G], shortcut)
            assert ok
            assert lengths.tolist() == w["lengths"][:G].tolist(), (name, shortcut, G)
            for k in range(G):
                assert np.array_equal(paths[k, :lengths[k]], w["paths"][k]), (name, shortcut, c["goals"][k])
        assert (w["lengths"] > 0).any() and (w["lengths"] == 0).any()
        # one short of the longest path as walked: -1 for it, the others as the harness has them under the same max_len
        raw = want[False]["lengths"]
        longest, n = int(np.argmax(raw)), int(raw.max())
        for room in (n - 1, n):
            paths, lengths, ok = _paths(gpu, c, got, c["goals"], shortcut, max_len=room)
            hp, hl = pc.harness_paths(plan_harness, w["field"], w["occ_plan"], c["start"], c["goals"], shortcut, max_len=room)
            assert ok and lengths.tolist() == hl.tolist() and (lengths[longest] == -1) == (room < n)
            assert (hl[raw < n] == w["lengths"][raw < n]).all()
            for k in range(21):
                assert np.array_equal(paths[k, :max(lengths[k], 0)], hp[k, :max(hl[k], 0)])


def test_goal_kinds_are_all_there(gpu, plan_harness):
    """what the cases above cover, said once: occupied, unreachable, next to the start, on the border, outside the grid"""
    c, want, _ = _planned(gpu, plan_harness, "70x67")
    w = want[False]
    by_goal = dict(zip(c["goals"], w["lengths"].tolist()))
    assert w["occ_plan"][20, 10] and by_goal[(20, 10)] == 0                       # occupied
    assert not w["occ_plan"][52, 50] and by_goal[(52, 50)] == 0                   # inside the island
    assert by_goal[(62, 10)] == 0 and by_goal[(21, 10)] == 0                      # under the Gaussian column; in the wall's dilation
    assert by_goal[(4, 3)] == 0 and by_goal[(3, 6)] == 2                          # the end cell is the start; one move away
    assert by_goal[(69, 66)] > 2 and by_goal[(0, 66)] > 2                         # corners of the border
    c, want, _ = _planned(gpu, plan_harness, "8x8")
    by_goal = dict(zip(c["goals"], want[True]["lengths"].tolist()))
    assert by_goal[(9, 3)] == 0 and by_goal[(-1, 0)] == 0 and by_goal[(5, 5)] == 0 and by_goal[(0, 0)] == 0
    assert by_goal[(0, 3)] == 3                                                   # two points, the last one twice under the shortcut


def test_no_gaussians_and_start_outside_free_space(gpu, plan_harness):
    c = _ragged()
    got = _field(gpu, c, points=None)
    occ, status = pc.harness_grid(plan_harness, c, points=None)
    assert got["intact"] and np.array_equal(got["occ_plan"], occ) and got["status"][1] == 0 and not got["occ_plan"][62, 10]
    c = pc.make_case("start-outside-free")
    got = _field(gpu, c)
    assert got["intact"] and got["status"][2] == 0 and got["status"][3] == 0 and (got["field"] == pc.UNREACHED).all()
    paths, lengths, ok = _paths(gpu, c, got, c["goals"], True)
    assert ok and not lengths.any()


def _planner(dev, c):
    from planning.astar import AstarPlanner
    p = AstarPlanner(device=dev)
    p.grid_dim = np.array([c["W"], c["H"]])
    p._map_center_np = np.asarray(c["center"], np.float64)
    p.map_center = torch.from_numpy(p._map_center_np).to(dev)
    p.cell_size = c["cell"]
    p.cam_height = c["cam_height"]
    p.occ_map = _dev(c["occ_map"], dev)
    return p


def test_python_layer(gpu, plan_harness, monkeypatch):
    from planning import astar
    c = _ragged()
    p = _planner(gpu, c)
    pts = _dev(c["points"], gpu)
    p._occ_cfg()                                                   # the map centre comes down once per map, not per call
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1])
    p.setup_start(np.array(c["start"]), pts, frame_idx=7)
    assert len(reads) == 1, reads                                  # the status; the convergence checks are counted by the library
    st = p.plan_stats
    assert st["convergence_reads"] >= 1 and st["rounds"] < st["rounds_launched"] and st["start_in_free_space"] and st["gaussians_binned"] == 101
    del reads[:]
    batch = p.plan_paths(np.array(c["goals"]))
    assert len(reads) == 1, reads
    del reads[:]
    single = [p.planning(np.array(g)) for g in c["goals"]]
    assert len(reads) == len(c["goals"])
    monkeypatch.undo()
    assert len(batch) == len(c["goals"]) and any(len(b) for b in batch) and any(len(b) == 0 for b in batch)
    for a, b in zip(batch, single):
        assert a.shape == b.shape and np.array_equal(a, b) and (a.ndim == 2 or a.shape == (0,))
    # the same through the harness on the grid and the free space the device built
    occ, status = pc.harness_grid(plan_harness, c)
    assert np.array_equal(p.occ_map_np, occ)
    free = p.free_space_np
    assert free.dtype == np.uint8 and free.shape == (c["H"], c["W"]) and free[c["start"]]
    field, _ = pc.harness_field(plan_harness, pc.harness_tiers(plan_harness, free), c["start"])
    cost, parent = p.plan_field()
    assert np.array_equal(cost.view(np.uint32), pc.field_cost(field).view(np.uint32))
    reached = field != pc.UNREACHED
    idx = (field & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert np.array_equal(parent[reached], np.stack([idx // c["W"], idx % c["W"]], -1)[reached]) and (parent[~reached] == -1).all()
    hp, hl = pc.harness_paths(plan_harness, field, occ, c["start"], c["goals"], True)
    for k, a in enumerate(batch):
        assert np.array_equal(a.reshape(-1, 2), hp[k, :hl[k]])
    # a path longer than the first call's room repeats the call and gives the same
    p.PLAN_MAX_LEN = 3
    again = p.plan_paths(np.array(c["goals"]))
    assert all(np.array_equal(a, b) for a, b in zip(batch, again))
    p.shortcut_path = False
    assert max(len(a) for a in p.plan_paths(np.array(c["goals"]))) > max(len(a) for a in batch)
    # all 8 neighbours occupied in the dilated map
    ring = pc.make_case("ring-8")
    q = _planner(gpu, ring)
    with pytest.raises(astar.LocalizationError, match="not in free space"):
        q.setup_start(ring["start"])
    q = _planner(gpu, pc.make_case("ring-7"))
    q.setup_start(pc.make_case("ring-7")["start"])
    assert q.plan_stats["ring"] == 7
