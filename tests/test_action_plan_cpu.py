"""Action planning on the CPU: the arithmetic (csrc/fr_action_math.h, compiled with g++ in tests/harness/fr_action_harness.cpp) against
the NumPy restatement of the reference loop in tests/action_cases.py on every case family -- action lists, counts, keep flags and cells
exactly, positions to 1e-12, the binary32 inverses to one ulp of float32(np.linalg.inv) -- each case's decision margin asserted first;
the roll-out against the planner and against path_eval's host roll-out; the stand-alone harness program under the address and
undefined-behaviour sanitizers; the ABI's rejections, which need no device; the Python wrappers' host logic on a stand-in library."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import action_cases as ac
import harness_build


@pytest.fixture(scope="module")
def harness():
    return ac.build_harness()


_CACHE = {}


def _computed(h, family):
    """the case, what the harness makes of it and what the restatement does -- once per family"""
    if family not in _CACHE:
        c = ac.make_case(family)
        _CACHE[family] = (c, ac.harness_plan(h, c), ac.np_action_planning(c))
    return _CACHE[family]


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_harness_equals_the_restatement(harness, family):
    c, got, want = _computed(harness, family)
    assert want["margin"] > ac.MARGIN, (family, want["margin"])
    worst_xz, worst_ulp = ac.compare(got, want, c)
    print(f"{family}: margin {want['margin']:.3g}  c2w_xz {worst_xz:.3g}  w2c ulps {worst_ulp}")
    assert got["n_actions"].max() <= c["Q"]


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_rollout_reproduces_the_plan_and_the_host_rollout(harness, family):
    from fisher_rast.path_eval import rollout
    c, got, want = _computed(harness, family)
    w2c, c2w = ac.harness_rollout(harness, ac.start_of(c), got["actions"], got["n_actions"], c["step"], c["turn"])
    assert np.array_equal(w2c.view(np.uint32), got["w2c"].view(np.uint32)), "the roll-out's inverses differ from the planner's"
    for g, n in enumerate(got["n_actions"]):
        n = max(int(n), 0)
        assert not c2w[g, n:].any()
        if n:
            assert np.abs(c2w[g, :n] - want["c2w"][g]).max() <= 1e-12
            assert np.abs(c2w[g, :n] - rollout(ac.start_of(c), want["actions"][g], c["step"], c["turn"])).max() <= 1e-12
            assert np.array_equal(c2w[g, :n, [0, 2], 3].T, got["c2w_xz"][g, :n])


def test_rollout_of_foreign_lists(harness):
    """lists that no planner made: the no-op actions 0 and 4, a negative count, the longest list there is"""
    from fisher_rast.path_eval import rollout
    rng = np.random.default_rng(5)
    Q = harness.fra_h_max_queue()
    assert Q >= 64
    acts = rng.integers(0, 5, size=(6, Q)).astype(np.uint8)
    n = np.array([Q, 0, -1, 17, 1, 64], np.int32)
    start = ac.yaw_pose(0.7, 1.5, 0.4, -2.25)
    for step, turn in ((0.065, 10.), (0.25, 30.)):
        w2c, c2w = ac.harness_rollout(harness, start, acts, n, step, turn)
        for g in range(6):
            k = max(int(n[g]), 0)
            assert not w2c[g, k:].any() and not c2w[g, k:].any()
            if k:
                want = rollout(start, acts[g, :k], step, turn)
                assert np.abs(c2w[g, :k] - want).max() <= 1e-12
                assert ac.ulp32(w2c[g, :k], np.linalg.inv(want).astype(np.float32)).max() <= 1


def test_the_families_sit_on_their_decisions(harness):
    # longer than the queue covers: the list is cut at Q, every action a step towards the goal
    c, got, want = _computed(harness, "corridor")
    assert want["n_actions"] == [c["Q"]] and want["actions"][0].count(1) > 10
    # the L-path is walked to its end: turns in the middle of the list, the re-orientation after the last forward step
    c, got, want = _computed(harness, "L-turn30")
    a = want["actions"][0]
    assert len(a) < c["Q"] and 1 in a and any(x != 1 for x in a[a.index(1):])
    # a path of one point: `finish` = (row, col) is appended into the x-z list as it is, so the agent heads for the cell (x = row, z = col)
    c, got, want = _computed(harness, "one-point")
    assert c["lengths"][0] == 1 and c["start"][0] != c["start"][1]
    swapped = dict(c, paths=c["paths"].copy(), lengths=c["lengths"].copy())
    swapped["paths"][0, 1] = c["goals"][0][::-1]                       # what an x-z append would have given: the start's neighbour
    swapped["lengths"][0] = 2
    assert ac.np_action_planning(swapped)["actions"][0] != want["actions"][0]
    assert want["n_actions"][0] == c["Q"]                              # the quirk's goal is far away
    # two points within one step, the goal's yaw within one turn: an empty list, which is a list -- the second one is a duplicate
    c, got, want = _computed(harness, "two-near")
    assert want["n_actions"] == [0, want["n_actions"][1], 0, -1] and want["n_actions"][1] > 0 and want["keep"] == [1, 1, 0, 0]
    # the wrap: the yaws differ by more than 180 degrees, the turn goes the short way round, in either direction
    for fam, first in (("wrap+", 3), ("wrap-", 2)):
        c, got, want = _computed(harness, fam)
        for g in (0, 1):
            d = np.rad2deg(np.arctan2(c["goals_c2w"][g][0, 2], c["goals_c2w"][g][2, 2])) - np.rad2deg(np.arctan2(c["agent"][0, 2], c["agent"][2, 2]))
            assert abs(d) > 180 and want["n_actions"][g] == int((360 - abs(d)) // c["turn"]) and set(want["actions"][g]) == {5 - first}
    # Q = 1 and 7; lengths 0 and -1 mixed in
    for fam in ("q1", "q7"):
        c, got, want = _computed(harness, fam)
        assert max(want["n_actions"]) == c["Q"] and want["n_actions"][2] == want["n_actions"][6] == -1 and sorted(c["lengths"][[2, 6]]) == [-1, 0]
    # duplicates: another path with the same list, and the same goal again
    c, got, want = _computed(harness, "dedupe")
    assert not np.array_equal(c["paths"][0], c["paths"][1]) and want["actions"][0] == want["actions"][1] and want["keep"][:2] == [1, 0]
    assert np.array_equal(c["paths"][0], c["paths"][3]) and want["keep"][3] == 0 and want["keep"][5:7] == [1, 0]
    # more goals than a wave has lanes, with a duplicate beyond the 64th
    c, got, want = _computed(harness, "g70")
    assert len(want["keep"]) == 70 and want["keep"][69] == 0 and want["n_actions"][69] >= 0 and sum(want["keep"]) > 20
    # the odd grid: grid_dim / 2 is a half cell, the centre is off the origin
    c, got, want = _computed(harness, "odd-grid")
    assert c["W"] % 2 == 1 and c["H"] % 2 == 1 and c["center"] != (0.0, 0.0)
    # the queue cap
    c, got, want = _computed(harness, "q-max")
    assert c["Q"] == harness.fra_h_max_queue()


def test_harness_program_under_sanitizers(tmp_path):
    """the stand-alone program (its own main) over the same header, under -fsanitize=address,undefined"""
    r = harness_build.sanitized_program("fr_action_harness", "FRA_HARNESS_MAIN", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checksum" in r.stdout and not r.stderr.strip()


def test_sources_exports_and_header(harness):
    from fisher_rast import _lib
    assert os.path.join(_lib._CSRC, "fr_action.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_action_math.h") in _lib.SOURCES
    header = open(os.path.join(ac.ROOT, "include", "fisher_occ.h")).read()
    for name in ("fr_plan_actions", "fr_rollout_actions"):
        assert name in _lib.EXPORTS and name + "(" in header
    assert f"#define FR_ACTION_MAX_QUEUE {_lib.FR_ACTION_MAX_QUEUE}" in header and _lib.FR_ACTION_MAX_QUEUE == harness.fra_h_max_queue() >= 64
    src = open(os.path.join(ac.ROOT, "fisher-nerf-customized_amd", "csrc", "fr_action.hip")).read()
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
    CAP = _lib.FR_ACTION_MAX_QUEUE

    def plan(cfg=ok, paths=A, max_len=8, lengths=A, goals=A, poses=A, G=2, agent=eye, h=0.4, step=0.065, turn=10., Q=30, cell=0.05, actions=A, n=A,
             keep=A, w2c=A, xz=A, cells=A):
        return lib.fr_plan_actions(ctypes.byref(cfg) if cfg else None, paths, max_len, lengths, goals, poses, G, agent, h, step, turn, Q, cell, actions,
                                   n, keep, w2c, xz, cells, None)

    def roll(start=eye, actions=A, n=A, G=2, Q=30, step=0.065, turn=10., w2c=A, c2w=A):
        return lib.fr_rollout_actions(start, actions, n, G, Q, step, turn, w2c, c2w, None)

    for call, name, bads in (
            (plan, b"fr_plan_actions", [dict(cfg=None), dict(cfg=_lib.OccCfg(0, 67, 0.05, 0, 0, 0, 0, 0)), dict(paths=None), dict(lengths=None), dict(goals=None),
                                        dict(poses=None), dict(actions=None), dict(n=None), dict(keep=None), dict(w2c=None), dict(xz=None), dict(cells=None),
                                        dict(agent=None), dict(agent=nan), dict(G=-1), dict(max_len=0), dict(Q=0), dict(Q=CAP + 1), dict(Q=-3),
                                        dict(step=0.0), dict(turn=0.0), dict(turn=float("nan")), dict(cell=0.0), dict(cell=float("inf")),
                                        dict(h=float("nan")), dict(paths=A + 2), dict(lengths=A + 1), dict(xz=A + 4), dict(n=A + 3), dict(w2c=A + 2)]),
            (roll, b"fr_rollout_actions", [dict(start=None), dict(start=nan), dict(actions=None), dict(n=None), dict(w2c=None), dict(G=-1), dict(Q=0),
                                           dict(Q=CAP + 1), dict(step=float("nan")), dict(turn=float("inf")), dict(n=A + 2), dict(w2c=A + 1), dict(c2w=A + 4)])):
        for bad in bads:
            assert call(**bad) == _lib.FR_EINVAL, (name, bad)
            assert name in lib.fr_last_error(), (name, bad)
    # nothing to do: no launch, whatever the pointers (a launch would fail here, there is no device)
    assert plan(G=0, paths=None, lengths=None, goals=None, poses=None, actions=None, n=None, keep=None, w2c=None, xz=None, cells=None) == _lib.FR_OK
    assert roll(G=0, actions=None, n=None, w2c=None, c2w=None) == _lib.FR_OK
    # but the cap holds with nothing to do as well
    assert plan(G=0, Q=CAP + 1) == _lib.FR_EINVAL and roll(G=0, Q=CAP + 1) == _lib.FR_EINVAL


# ---- the Python layer on a stand-in library: the harness behind the two entry points, the planner's tensors on the host -------------------------

class _StandInLib:
    """fr_plan_paths hands out a case's paths (-1 where one does not fit max_len), fr_plan_actions is the g++ harness"""

    def __init__(self, h, c):
        self.h, self.c, self.calls = h, c, []

    def fr_plan_paths(self, cfg, field, occ, sy, sx, goals, G, shortcut, paths, max_len, lengths, stream):
        c = self.c
        self.calls.append(("fr_plan_paths", max_len))
        assert G == len(c["lengths"]) and (sy, sx) == (c["start"][1], c["start"][0])
        out_p = np.ctypeslib.as_array(ctypes.cast(paths, ctypes.POINTER(ctypes.c_int32)), (G, max_len, 2))
        out_n = np.ctypeslib.as_array(ctypes.cast(lengths, ctypes.POINTER(ctypes.c_int32)), (G,))
        for g, n in enumerate(c["lengths"]):
            if n > max_len:
                out_n[g] = -1
            else:
                out_n[g] = max(int(n), 0)
                out_p[g, :max(int(n), 0)] = c["paths"][g, :max(int(n), 0)]
        return 0

    def fr_plan_actions(self, cfg, paths, max_len, lengths, goals, poses, G, agent, height, step, turn, Q, cell, actions, n, keep, w2c, xz, cells, stream):
        self.calls.append(("fr_plan_actions", max_len))
        o = cfg._obj
        self.h.fra_h_plan(o.grid_w, o.grid_h, cell, o.center_x, o.center_z, paths, max_len, lengths, goals, poses, G, ctypes.addressof(agent), height, step,
                          turn, Q, actions, n, keep, w2c, xz, cells)
        return 0


def _stand_in_planner(monkeypatch, h, c):
    from fisher_rast import _lib
    from planning import AstarPlanner
    fake = _StandInLib(h, c)
    monkeypatch.setattr(_lib, "load", lambda: fake)
    pl = AstarPlanner(device="cpu", cell_size=c["cell"])
    pl.grid_dim = np.array([c["W"], c["H"]])
    pl.map_center = torch.tensor(c["center"], dtype=torch.float32)
    pl.cam_height = c["cam_height"]
    pl._stream = lambda: None
    sx, sz = c["start"]
    pl._plan = dict(cfg=pl._occ_cfg(), start=(sz, sx), field=torch.zeros(1, dtype=torch.int64), occ_plan=torch.zeros(1, dtype=torch.uint8))
    reads = []
    pl._plan_read = lambda t: (reads.append(tuple(t.shape)), t.cpu().numpy())[1]
    return pl, fake, reads


def _goal_poses_at_finish(c):
    """the case's goal poses are at their finish cells' centres: the wrapper's own conversion gives the case's goal cells back"""
    pol = ac.Policy(c)
    for g, pose in enumerate(c["goals_c2w"]):
        assert pol.convert_to_map(pose[[0, 2], 3])[[1, 0]].tolist() == c["goals"][g].tolist()


@pytest.mark.parametrize("family", ["odd-grid", "dedupe", "one-point", "all-without-path"])
def test_plan_actions_host_logic_on_a_stand_in_library(monkeypatch, harness, family):
    c, _, want = _computed(harness, family)
    _goal_poses_at_finish(c)
    pl, fake, reads = _stand_in_planner(monkeypatch, harness, c)
    plan = pl.plan_actions(c["goals_c2w"], c["agent"], forward_step_size=c["step"], turn_angle=c["turn"], queue_size=c["Q"])
    assert len(reads) == 1 and plan.reads == 1 and [n for n, _ in fake.calls] == ["fr_plan_paths", "fr_plan_actions"]
    assert plan.kept_index == want["kept_index"] and plan.path_actions == want["path_actions"]
    assert plan.n_actions.tolist() == want["n_actions"] and plan.keep.tolist() == want["keep"]
    vg, pa, arr = plan.triple()
    assert len(vg) == len(pa) == len(arr) == len(want["kept_index"])
    for k, g in enumerate(want["kept_index"]):
        assert np.array_equal(vg[k], c["goals_c2w"][g]) and np.array_equal(arr[k], want["paths_arr"][k])
        assert [m.tolist() for m in plan.map_path[k]] == [m.tolist() for m in want["map_path"][g]]
        assert len(plan.world_path[k]) == len(want["world_path"][g])
        if plan.world_path[k]:
            assert np.abs(np.array(plan.world_path[k]) - np.array(want["world_path"][g])).max() <= 1e-12
    assert plan.w2c.shape == (len(c["lengths"]), c["Q"], 4, 4) and plan.kept_w2c().shape[0] == len(want["kept_index"])
    assert [len(p) for p in plan.paths] == [max(int(n), 0) for n in c["lengths"]]
    # the map centre is not fetched per goal: once it is held, a call brings one tensor to the host, the packed buffer
    fetched = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (fetched.append(tuple(self.shape)), real(self, *a, **k))[1])
    pl.plan_actions(c["goals_c2w"], c["agent"], forward_step_size=c["step"], turn_angle=c["turn"], queue_size=c["Q"])
    assert len(fetched) == (1 if len(c["lengths"]) else 0) and fetched[0][0] > 2, fetched


def test_plan_actions_repeats_once_for_a_long_path_and_validates(monkeypatch, harness):
    c, _, want = _computed(harness, "L-turn30")
    pl, fake, reads = _stand_in_planner(monkeypatch, harness, c)
    pl.PLAN_MAX_LEN = 2                                        # the L-paths have three points
    kw = dict(forward_step_size=c["step"], turn_angle=c["turn"], queue_size=c["Q"])
    plan = pl.plan_actions(torch.from_numpy(c["goals_c2w"]), torch.from_numpy(c["agent"]), **kw)
    assert fake.calls == [("fr_plan_paths", 2), ("fr_plan_actions", 2), ("fr_plan_paths", c["W"] * c["H"] + 1), ("fr_plan_actions", c["W"] * c["H"] + 1)]
    assert plan.reads == 2 == len(reads) and plan.path_actions == want["path_actions"]
    # no goals: nothing is called or read
    fake.calls.clear()
    empty = pl.plan_actions(np.zeros((0, 4, 4), np.float32), c["agent"], **kw)
    assert empty.triple() == ([], [], []) and empty.reads == 0 and not fake.calls and empty.w2c.shape == (0, c["Q"], 4, 4)
    from fisher_rast import _lib
    for bad in (dict(kw, queue_size=0), dict(kw, queue_size=_lib.FR_ACTION_MAX_QUEUE + 1), dict(kw, forward_step_size=0.0), dict(kw, turn_angle=-10.)):
        with pytest.raises(ValueError):
            pl.plan_actions(c["goals_c2w"], c["agent"], **bad)
    with pytest.raises(ValueError, match="4 x 4"):
        pl.plan_actions(c["goals_c2w"], c["agent"][:3], **kw)
    moved = c["agent"].copy()
    moved[0, 3] += 3 * c["cell"]
    with pytest.raises(ValueError, match="setup_start"):
        pl.plan_actions(c["goals_c2w"], moved, **kw)
    assert not fake.calls


def test_install_carries_plan_actions_and_leaves_the_reference_conversions():
    from planning import astar
    keep = lambda self, coord: None
    cls = type("RefPlanner", (), {"convert_to_map": keep})
    astar.PathPlanOps.install(cls)
    assert cls.plan_actions is astar.PathPlanOps.__dict__["plan_actions"] and cls.convert_to_map is keep
    assert cls.convert_to_world is astar.PathPlanOps.__dict__["convert_to_world"]


def test_poses_w2c_and_rollout_device_argument_errors():
    from fisher_rast import _lib, path_eval
    scorer = types.SimpleNamespace(dev=torch.device("cpu"), P=4, columns=4)
    paths = [[1, 2, 1], [3]]
    args = (scorer, np.eye(4), paths, [0.0, 0.0], torch.zeros((4, 4)))
    for bad in (np.zeros((2, 3, 4, 4), np.float32), torch.zeros((3, 3, 4, 4)), torch.zeros((2, 2, 4, 4)), torch.zeros((2, 3, 16)), torch.zeros((2, 3, 4, 4), dtype=torch.float64),
                torch.zeros((2, 3, 3, 4))):
        with pytest.raises(ValueError, match="poses_w2c"):
            path_eval.evaluate_paths(*args, poses_w2c=bad)
        slam = types.SimpleNamespace(params={"means3D": torch.zeros((4, 3))})
        with pytest.raises(ValueError, match="poses_w2c"):
            path_eval.evaluate_paths_popgs(slam, np.eye(4), paths, [0.0, 0.0], torch.zeros(44), poses_w2c=bad)
    # no accumulation step, so no launch: the value is the end term alone, with or without the device poses
    short = [[1], [2, 3]]
    with_poses = path_eval.evaluate_paths(scorer, np.eye(4), short, [0.5, 0.25], torch.zeros((4, 4)), acc_H_train_every=5, poses_w2c=torch.zeros((2, 2, 4, 4)))
    assert with_poses == path_eval.evaluate_paths(scorer, np.eye(4), short, [0.5, 0.25], torch.zeros((4, 4)), acc_H_train_every=5) == [0.5, 0.125]
    for bad in (dict(path_actions=[[1] * (_lib.FR_ACTION_MAX_QUEUE + 1)]), dict(path_actions=[[1, 2, 3]], queue_size=2), dict(path_actions=[[1, 300]]),
                dict(path_actions=[[1]], start_c2w=np.eye(3))):
        kw = dict(start_c2w=np.eye(4), device="cpu")
        kw.update(bad)
        with pytest.raises(ValueError):
            path_eval.rollout_device(kw.pop("start_c2w"), kw.pop("path_actions"), **kw)


def test_step_configuration_of_the_round():
    from fisher_rast import plan_round
    want = dict(forward_step_size=0.065, turn_angle=10, queue_size=30)
    assert plan_round._step_cfg(want) == want
    assert plan_round._step_cfg(dict(forward_step_size=0.065, turn_angle=10, policy=dict(planning_queue_size=30), other=1)) == want
    assert plan_round._step_cfg(dict(forward_step_size=0.065, turn_angle=10, planning_queue_size=30)) == want
    with pytest.raises(ValueError, match="queue_size"):
        plan_round._step_cfg(dict(forward_step_size=0.065, turn_angle=10))
