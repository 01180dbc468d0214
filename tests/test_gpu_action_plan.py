"""-m gpu: action planning on the device (fr_plan_actions / fr_rollout_actions, csrc/fr_action.hip) and the Python layer on it
(planning/astar.py: PathPlanOps.plan_actions; fisher_rast/path_eval.py: rollout_device, poses_w2c=; fisher_rast/plan_round.py).

Through the C ABI on guarded buffers over every case family of tests/action_cases.py, against the g++ harness over the same header
(tests/harness/fr_action_harness.cpp) and the NumPy restatement of the reference loop: action lists, counts, keep flags and cells equal,
positions to 1e-12, the binary32 inverses to one ulp; zeros behind every list; guards intact; the roll-out kernel reproduces the
planner's inverses bit for bit; the same on a non-default stream; the queue cap and G = 0 refused or accepted without a launch.
Through the Python layer: plan_actions on a 96 x 96 two-room map against plan_paths fed to the restatement, one host read;
evaluate_paths with the device poses against evaluate_paths with its host roll-out; plan_best_path's choice and shapes."""
import ctypes

import numpy as np
import pytest
import torch

import action_cases as ac

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes behind every buffer
GUARD_BYTE = 0x5A


@pytest.fixture(scope="module")
def harness():
    return ac.build_harness()


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


def _cfg(c):
    from fisher_rast import _lib
    return _lib.OccCfg(c["W"], c["H"], c["cell"], c["center"][0], c["center"][1], -0.6, 0.6, 10.0)


def _f64x16(m):
    return (ctypes.c_double * 16)(*[float(v) for v in np.asarray(m, np.float64).reshape(-1)])


def _device_plan(dev, c, staged=None):
    """fr_plan_actions, then fr_rollout_actions over its lists, on guarded buffers on the current stream:
    dict(the layout of ac.harness_plan, roll_w2c, roll_c2w, intact).  staged: the inputs already on the device (made in stream order)."""
    from fisher_rast import _lib
    lib = _lib.load()
    a = ac.case_arrays(c)
    G, Q = len(a["lengths"]), c["Q"]
    d = staged if staged is not None else {k: torch.from_numpy(a[k]).to(dev) for k in ("paths", "lengths", "goals", "goals_c2w")}
    b = dict(actions=_Guarded(G * Q, dev), n=_Guarded(4 * G, dev), keep=_Guarded(G, dev), w2c=_Guarded(64 * G * Q, dev), xz=_Guarded(16 * G * Q, dev),
             cells=_Guarded(8 * G * Q, dev), roll_w2c=_Guarded(64 * G * Q, dev), roll_c2w=_Guarded(128 * G * Q, dev))
    cfg = _cfg(c)
    _lib.check(lib.fr_plan_actions(ctypes.byref(cfg), d["paths"].data_ptr(), c["max_len"], d["lengths"].data_ptr(), d["goals"].data_ptr(),
                                   d["goals_c2w"].data_ptr(), G, _f64x16(c["agent"]), c["cam_height"], c["step"], c["turn"], Q, c["cell"], b["actions"].ptr,
                                   b["n"].ptr, b["keep"].ptr, b["w2c"].ptr, b["xz"].ptr, b["cells"].ptr, _stream(dev)), "fr_plan_actions")
    _lib.check(lib.fr_rollout_actions(_f64x16(ac.start_of(c)), b["actions"].ptr, b["n"].ptr, G, Q, c["step"], c["turn"], b["roll_w2c"].ptr,
                                      b["roll_c2w"].ptr, _stream(dev)), "fr_rollout_actions")
    torch.cuda.current_stream(dev).synchronize()
    return dict(actions=b["actions"].get(np.uint8).reshape(G, Q), n_actions=b["n"].get(np.int32), keep=b["keep"].get(np.uint8),
                w2c=b["w2c"].get(np.float32).reshape(G, Q, 4, 4), c2w_xz=b["xz"].get(np.float64).reshape(G, Q, 2),
                map_xz=b["cells"].get(np.int32).reshape(G, Q, 2), roll_w2c=b["roll_w2c"].get(np.float32).reshape(G, Q, 4, 4),
                roll_c2w=b["roll_c2w"].get(np.float64).reshape(G, Q, 4, 4), intact=all(g.intact() for g in b.values()))


_WANT = {}


def _expected(h, family):
    """the case, the harness's answer and the restatement's -- once per family, shared by the tests, never written to"""
    if family not in _WANT:
        c = ac.make_case(family)
        _WANT[family] = (c, ac.harness_plan(h, c), ac.np_action_planning(c))
    return _WANT[family]


def _check(c, got, hw, want):
    assert got["intact"], "a guard behind an output was written"
    ac.compare(got, want, c)                                  # the margin first, then the restatement by the issue's rules
    # and the harness over the same header: everything decided equal, the numbers within the same bounds
    for k in ("actions", "n_actions", "keep", "map_xz"):
        assert np.array_equal(got[k], hw[k]), (c["name"], k)
    assert np.abs(got["c2w_xz"] - hw["c2w_xz"]).max(initial=0.0) <= 1e-12
    assert ac.ulp32(got["w2c"], hw["w2c"]).max(initial=0) <= 1
    # the two kernels agree: rolling the planned actions out reproduces the planner's inverses bit for bit
    assert np.array_equal(got["roll_w2c"].view(np.uint32), got["w2c"].view(np.uint32))
    for g, n in enumerate(got["n_actions"]):
        n = max(int(n), 0)
        assert not got["roll_c2w"][g, n:].any()
        if n:
            assert np.abs(got["roll_c2w"][g, :n] - want["c2w"][g]).max() <= 1e-12


@pytest.mark.parametrize("family", ac.FAMILIES)
def test_device_equals_harness_and_restatement(gpu, harness, family):
    c, hw, want = _expected(harness, family)
    _check(c, _device_plan(gpu, c), hw, want)


@pytest.mark.parametrize("family", ["g70", "odd-grid"])
def test_on_a_side_stream_in_stream_order(gpu, harness, family):
    c, hw, want = _expected(harness, family)
    a = ac.case_arrays(c)
    host = {k: torch.from_numpy(a[k]).pin_memory() for k in ("paths", "lengths", "goals", "goals_c2w")}
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        # the inputs arrive on the side stream, behind a device-side detour: the kernels can only be right if they wait for them
        staged = {k: (v.to(gpu, non_blocking=True).clone().flip(0).flip(0)).contiguous() for k, v in host.items()}
        got = _device_plan(gpu, c, staged)
    _check(c, got, hw, want)


def test_cap_and_empty_call_return_without_a_launch(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    c = ac.make_case("corridor")
    cfg = _cfg(c)
    eye = _f64x16(np.eye(4))
    out = _Guarded(4096, gpu)
    CAP = _lib.FR_ACTION_MAX_QUEUE
    p = out.ptr
    torch.cuda.synchronize()
    assert lib.fr_plan_actions(ctypes.byref(cfg), p, 4, p, p, p, 1, eye, 0.4, 0.065, 10., CAP + 1, 0.05, p, p, p, p, p, p, _stream(gpu)) == _lib.FR_EINVAL
    assert b"queue_size" in lib.fr_last_error()
    assert lib.fr_rollout_actions(eye, p, p, 1, CAP + 1, 0.065, 10., p, p, _stream(gpu)) == _lib.FR_EINVAL
    assert lib.fr_plan_actions(ctypes.byref(cfg), None, 4, None, None, None, 0, eye, 0.4, 0.065, 10., 30, 0.05, None, None, None, None, None, None,
                               _stream(gpu)) == _lib.FR_OK
    assert lib.fr_rollout_actions(eye, None, None, 0, 30, 0.065, 10., None, None, _stream(gpu)) == _lib.FR_OK
    torch.cuda.synchronize()
    assert bool((out.buf == GUARD_BYTE).all())


# ---- the Python layer --------------------------------------------------------------------------------------------------------------------

STEP = dict(forward_step_size=0.25, turn_angle=30., queue_size=30)


@pytest.fixture(scope="module")
def two_rooms(gpu):
    """96 x 96 cells of 5 cm: two rooms, a wall between them with a door, unknown cells round them; the agent in the left room; 12 goals --
    in both rooms, in the wall, next to the agent, one of them twice.  dict(planner, c (a case for the restatement), goal_c2ws)"""
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
    c = dict(name="two-rooms", W=W, H=H, cell=0.05, center=(0.0, 0.0), turn=STEP["turn_angle"], step=STEP["forward_step_size"], Q=STEP["queue_size"],
             cam_height=0.4, start=(20, 30))
    pol = ac.Policy(c)
    rng = np.random.default_rng(21)
    pos = pol.world_at(np.array([20.5, 30.5]) + rng.uniform(-0.2, 0.2, 2))
    c["agent"] = ac.yaw_pose(rng.uniform(-np.pi, np.pi), pos[0], 1.1, pos[1])
    cells = [(70, 20), (30, 75), (60, 80), (46, 70), (30, 48), (30, 21), (70, 20), (15, 40), (80, 60), (2, 2), (45, 30), (12, 84)]     # (row, col)
    goal_c2ws = np.zeros((len(cells), 4, 4), np.float32)
    for g, (row, col) in enumerate(cells):
        w = pol.world_at(np.array([col, row]) + 0.5)
        goal_c2ws[g] = ac.yaw_pose(rng.uniform(-np.pi, np.pi), w[0], rng.uniform(0.2, 1.5), w[1], np.float32)
    goal_c2ws[6] = goal_c2ws[0]                                  # the same goal twice: cell and pose
    c["goals"] = np.array(cells, np.int32)
    c["goals_c2w"] = goal_c2ws
    p = AstarPlanner(device=gpu)
    p.grid_dim = np.array([W, H])
    p._map_center_np = np.zeros(2)
    p.map_center = torch.from_numpy(p._map_center_np).to(gpu)
    p.cell_size = c["cell"]
    p.cam_height = c["cam_height"]
    p.occ_map = torch.from_numpy(occ_map).to(gpu)
    return dict(planner=p, c=c, goal_c2ws=goal_c2ws)


def test_plan_actions_equals_plan_paths_fed_to_the_restatement(gpu, two_rooms, monkeypatch):
    p, c, goal_c2ws = two_rooms["planner"], two_rooms["c"], two_rooms["goal_c2ws"]
    p.setup_start(np.array([c["start"][1], c["start"][0]]))
    paths = p.plan_paths(c["goals"])
    want = ac.np_action_planning(c, paths_list=paths)
    assert want["margin"] > ac.MARGIN, want["margin"]
    assert want["n_actions"][4] == -1 and want["n_actions"][9] == -1 and want["keep"][6] == 0 and sum(want["keep"]) >= 6        # wall, unknown, twice
    reads = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append(tuple(self.shape)), real(self, *a, **k))[1])
    plan = p.plan_actions(goal_c2ws, c["agent"], **STEP)
    monkeypatch.undo()
    assert len(reads) == 1 and plan.reads == 1, reads                    # one read for the actions, none for the poses
    assert plan.w2c.is_cuda and plan.w2c.shape == (12, 30, 4, 4)
    assert plan.n_actions.tolist() == want["n_actions"] and plan.keep.tolist() == want["keep"]
    assert plan.kept_index == want["kept_index"] and plan.path_actions == want["path_actions"]
    for a, b in zip(plan.paths, paths):
        assert np.array_equal(a, b)
    vg, pa, arr = plan.triple()
    w2c = plan.w2c.cpu().numpy()
    for k, g in enumerate(want["kept_index"]):
        n = want["n_actions"][g]
        assert np.array_equal(vg[k], goal_c2ws[g]) and np.array_equal(arr[k], want["paths_arr"][k])
        assert [m.tolist() for m in plan.map_path[k]] == [m.tolist() for m in want["map_path"][g]]
        assert len(plan.world_path[k]) == len(want["world_path"][g])
        if plan.world_path[k]:
            assert np.abs(np.array(plan.world_path[k]) - np.array(want["world_path"][g])).max() <= 1e-12
        if n:
            assert ac.ulp32(w2c[g, :n], np.linalg.inv(want["c2w"][g]).astype(np.float32)).max() <= 1
        assert not w2c[g, n:].any()
    # the round's first half as the reference returns it
    from fisher_rast import plan_round
    triple = plan_round.action_planning(p, goal_c2ws, c["agent"], None, 3, **STEP)
    assert triple[1] == want["path_actions"] and len(triple[0]) == len(triple[2]) == len(want["kept_index"])
    # a path longer than the first call's room repeats both calls and the read, and gives the same
    p.PLAN_MAX_LEN = 2
    again = p.plan_actions(goal_c2ws, c["agent"], **STEP)
    del p.PLAN_MAX_LEN
    assert again.reads == 2 and again.path_actions == plan.path_actions and torch.equal(again.w2c, plan.w2c)


@pytest.fixture(scope="module")
def small_map(gpu):
    """a 2 000-Gaussian room shell at 64 x 64 with two keyframes folded into H_train"""
    from fisher_rast import synthetic
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    P, W, H = 2000, 64, 64
    act = synthetic.activate(synthetic.room_shell(P, seed=9))
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    sc = FisherScorer(cam, *(act[k].to(gpu) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")))
    H_train = torch.zeros((P, sc.columns), device=gpu)
    sc.run(synthetic.invert_rigid(synthetic.candidate_poses(2, seed=10)).to(gpu), out_H=H_train)
    return sc, H_train


def test_evaluate_paths_with_device_poses_equals_the_host_rollout(gpu, small_map):
    from fisher_rast.path_eval import evaluate_paths, rollout_device
    sc, H_train = small_map
    start = ac.yaw_pose(0.83, 0.4, 0.0, -1.3)
    rng = np.random.default_rng(3)
    paths = [[int(a) for a in rng.integers(1, 4, size=n)] for n in (9, 4, 3, 7, 12)]     # one path has no accumulation step at acc = 4
    finals = [0.3, -0.1, 0.7, 0.2, 0.0]
    w2c, lengths = rollout_device(start, paths, 0.065, 10., device=gpu)
    assert w2c.shape == (5, 12, 4, 4) and lengths == [9, 4, 3, 7, 12]
    for acc, w_end, fisher in ((4, 0.0, False), (2, 0.5, False), (4, 0.0, True)):
        kw = dict(H_reg_lambda=0.1, acc_H_train_every=acc, path_point_weight=1.0, path_pose_weight=0.05 if fisher else 0.0, path_end_weight=w_end,
                  pose_fisher=fisher, pose_reg=1e-3)
        want = evaluate_paths(sc, start, paths, finals, H_train, **kw)
        got = evaluate_paths(sc, start, paths, finals, H_train, poses_w2c=w2c, **kw)
        print(f"acc {acc} end {w_end} pose_fisher {fisher}: max rel diff {np.max(np.abs(np.array(got) - want) / np.abs(want)):.3g}")
        assert np.allclose(got, want, rtol=1e-5, atol=0), (got, want)


def test_plan_best_path_takes_the_argmax_and_keeps_the_reference_shapes(gpu, two_rooms, small_map):
    from fisher_rast import plan_round
    from fisher_rast.path_eval import evaluate_paths
    sc, H_train = small_map
    p, c, goal_c2ws = two_rooms["planner"], two_rooms["c"], two_rooms["goal_c2ws"]
    rng = np.random.default_rng(8)
    EIGs = torch.from_numpy(rng.uniform(0.5, 3.0, len(goal_c2ws)).astype(np.float32))
    cfg = dict(STEP, H_reg_lambda=0.1, acc_H_train_every=5, path_point_weight=1.0, path_end_weight=0.0)
    for align in (False, True):
        res = plan_round.plan_best_path(sc, p, torch.from_numpy(goal_c2ws).to(gpu), EIGs, H_train, c["agent"], None, 0, cfg, align_EIGs=align)
        best_path, best_map_path, best_goal, best_world_path, best_global_path, totals = res
        plan = res.plan
        order = np.argsort(EIGs.numpy())[::-1]
        assert np.array_equal(res.global_points, goal_c2ws[order]) and np.array_equal(res.EIGs, EIGs.numpy()[order])
        assert len(totals) == len(res.scored) <= plan_round.MAX_SCORED_PATHS and len(res.scored) + len(res.skipped_empty) == len(plan.kept_index) >= 6
        assert all(len(plan.path_actions[i]) == 0 for i in res.skipped_empty) and all(np.isfinite(totals))
        finals = [float(res.EIGs[plan.kept_index[i]] if align else res.EIGs[i]) for i in res.scored]
        want = evaluate_paths(sc, c["agent"], [plan.path_actions[i] for i in res.scored], finals, H_train, cam_height=c["cam_height"],
                              forward_step_size=STEP["forward_step_size"], turn_angle=STEP["turn_angle"], H_reg_lambda=0.1, acc_H_train_every=5)
        assert np.allclose(totals, want, rtol=1e-5, atol=0)
        assert max(totals) > -1 and res.best_index == res.scored[int(np.argmax(totals))]
        k = res.best_index
        assert best_path == plan.path_actions[k] and all(isinstance(a, int) for a in best_path)
        assert best_goal.shape == (4, 4) and np.array_equal(best_goal, res.global_points[plan.kept_index[k]])
        assert best_global_path.ndim == 2 and best_global_path.shape[1] == 2
        assert len(best_map_path) == len(best_world_path) == best_path.count(1)
        assert all(m.shape == (2,) and w.shape == (2,) for m, w in zip(best_map_path, best_world_path))
