"""-m gpu: DBSCAN and the target selection on the device (csrc/fr_cluster.hip through fisher_rast/cluster.py, a thin layer over the C
ABI).  Labels must be array_equal to the g++ harness over the same header (tests/harness/fr_cluster_harness.cpp), to the float64
restatement of tests/cluster_cases.py and to sklearn's recorded labels (tests/golden/dbscan_cases.npz) on every case family: sizes
at wave and workgroup edges, a 2000-point chain, two clusters joined only by a border point, a permuted cloud, pairs straddling
cell edges, an exactly representable distance, 4096 points in one ball, a far outlier, non-finite rows, min_samples 1 and beyond N;
two calls give the same bits; one run on a non-default stream by the procedure of tests/stream_cases.py.  select_target against the
harness and against the torch + restatement chain on a 20k-point synthetic map, with its edge cases; global_planning on the
product's GaussianSLAM with stub frontiers, candidates and follower against a loop over per-view compute_Hessian."""
import functools
import os

import numpy as np
import pytest
import torch

import cluster_cases as kc
import stream_cases as sc

pytestmark = pytest.mark.gpu

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dbscan_cases.npz")


@functools.lru_cache(maxsize=None)
def _case(family, N, eps, ms):
    """the cloud and the three statements of its labels, computed once and shared (read-only)"""
    pts, seed = kc.qualifying_case(family, N, eps)
    labels, status = kc.harness_dbscan(kc.build_harness(), pts, eps, ms)
    assert np.array_equal(labels, kc.restate_dbscan(pts, eps, ms))
    assert np.array_equal(labels, np.load(GOLDEN)[f"{family}/{N}/{eps:g}/{ms}/labels"].astype(np.int32))
    for a in (pts, labels, status):
        a.setflags(write=False)
    return pts, labels, status


def _run(pts, gpu, eps=kc.EPS, ms=kc.MIN_SAMPLES):
    from fisher_rast.cluster import dbscan_raw
    labels, status = dbscan_raw(torch.from_numpy(np.array(pts, F)).reshape(-1, 3).to(gpu), eps, ms)
    return labels.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("family,N,eps,ms", kc.GOLDEN)
def test_labels_equal_harness_restatement_and_recorded_sklearn(gpu, family, N, eps, ms):
    pts, want, want_status = _case(family, N, eps, ms)
    labels, status = _run(pts, gpu, eps, ms)
    assert labels.dtype == np.int32 and np.array_equal(labels, want), (family, N, int((labels != want).sum()))
    assert np.array_equal(status, want_status)                       # clusters, finite points, the three cell sides bit for bit


def test_empty_and_small_clouds(gpu):
    labels, status = _run(np.zeros((0, 3), F), gpu)
    assert labels.shape == (0,) and not status.any()
    assert _run(kc.make_case("tiny", 1), gpu)[0].tolist() == [-1]
    assert _run(kc.make_case("tiny", 4), gpu)[0].tolist() == [-1] * 4                    # below min_samples
    assert _run(kc.make_case("tiny", 5), gpu)[0].tolist() == [0] * 5                     # five identical points
    assert _run(kc.make_case("tiny", 4), gpu, ms=1)[0].tolist() == [0] * 4
    assert _run(kc.make_case("tiny", 1), gpu, ms=1)[0].tolist() == [0]


def test_border_point_between_two_clusters(gpu):
    pts = kc.make_case("bridge", 17)
    labels, status = _run(pts, gpu)
    assert status[0] == 2 and labels[:8].tolist() == [0] * 8 and labels[9:].tolist() == [1] * 8 and labels[8] == 0
    labels, _ = _run(pts[::-1].copy(), gpu)
    assert labels[:8].tolist() == [0] * 8 and labels[9:].tolist() == [1] * 8 and labels[8] == 0


def test_permutation_keeps_the_partition(gpu):
    pts, want, _ = _case("permuted", 1025, kc.EPS, kc.MIN_SAMPLES)
    perm = np.random.default_rng(5).permutation(len(pts))
    got = _run(pts[perm], gpu)[0]
    assert kc.same_partition(want[perm], got)
    assert np.array_equal(got, kc.harness_dbscan(kc.build_harness(), pts[perm])[0])      # numbered by the lowest core index of the new order


def test_inclusive_at_an_exactly_representable_distance(gpu):
    pts = np.array([[0, 0, 0], [0.125, 0, 0], [0.25, 0, 0], [0.25, 0.1250001, 0]], F)
    assert _run(pts, gpu, 0.125, 2)[0].tolist() == [0, 0, 0, -1]
    assert _run(pts - F(7.0), gpu, 0.125, 2)[0].tolist() == kc.harness_dbscan(kc.build_harness(), pts - F(7.0), 0.125, 2)[0].tolist()


def test_wide_clouds_get_larger_cells_and_the_same_labels(gpu):
    """beyond 1024 cells of 1.125 eps an axis is coarsened (status reports it); the labels do not change"""
    pts, want, _ = _case("blobs", 1025, kc.EPS, kc.MIN_SAMPLES)
    far = np.concatenate([pts, np.array([[1e6, 3.0, -2e5], [np.inf, 0, 0], [0, np.nan, 0]], F)])
    labels, status = _run(far, gpu)
    assert np.array_equal(labels[:-3], want) and labels[-3:].tolist() == [-1, -1, -1]
    sides = status[2:5].copy().view(F)
    assert sides[0] > 900 and sides[1] == F(0.1) * F(1.125) and sides[2] > 190 and status[1] == len(pts) + 1
    assert np.array_equal(status, kc.harness_dbscan(kc.build_harness(), far)[1])


def test_two_calls_give_the_same_bits(gpu):
    pts, want, _ = _case("blobs", 5000, kc.EPS, kc.MIN_SAMPLES)
    a, b = _run(pts, gpu), _run(pts, gpu)
    assert a[0].tobytes() == b[0].tobytes() == want.tobytes() and a[1].tobytes() == b[1].tobytes()


def test_numpy_and_float64_inputs(gpu):
    from fisher_rast.cluster import dbscan_labels
    pts, want, _ = _case("blobs", 257, kc.EPS, kc.MIN_SAMPLES)
    for x in (pts, pts.astype(np.float64), torch.from_numpy(np.array(pts)), torch.from_numpy(np.array(pts)).to(gpu).double()):
        got = dbscan_labels(x)
        assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)


def test_on_a_non_default_stream(gpu):
    """both entry points behind a blocker on a stream that runs beside the default stream: only stream order gives the result"""
    def make(which):
        means, scores = kc.make_select_case(5000, seed=which)
        return dict(points=kc.make_case("blobs", 1025, seed=which), means=means, scores=scores)

    def call(ctx, b):
        from fisher_rast.cluster import dbscan_raw
        from fisher_rast import _lib
        from fisher_rast.ops import _ptr, _stream
        labels, status = dbscan_raw(b["points"])
        # fr_target_select through the C ABI (select_target reads the status block on the host, which would wait for the blocker)
        lib, dev, P = _lib.load(), b["means"].device, int(b["means"].shape[0])
        lists = torch.zeros((4, P), dtype=torch.int32, device=dev)
        st = torch.zeros((_lib.FR_TARGET_STATUS_WORDS,), dtype=torch.int32, device=dev)
        thr = torch.zeros((1,), dtype=torch.float32, device=dev)
        ws = torch.empty((int(lib.fr_target_select_workspace_bytes(P)) // 8,), dtype=torch.int64, device=dev)
        _lib.check(lib.fr_target_select(P, _ptr(b["means"]), _ptr(b["scores"]), kc.LOWER_Y, kc.UPPER_Y, kc.Q, kc.EPS, kc.MIN_SAMPLES, _ptr(lists[0]),
                                        _ptr(lists[1]), _ptr(lists[2]), _ptr(lists[3]), _ptr(thr), _ptr(st), _ptr(ws), ws.numel() * 8, _stream(dev)),
                   "fr_target_select")
        return dict(labels=labels, select_status=st, threshold=thr, band=lists[0, :256])
    case = sc.Case(name="cluster_dbscan_target_select", make=make, call=call, exact=("labels", "select_status", "threshold", "band"), sync_free=True)
    ref, got = sc.run_case(case, gpu)
    h = kc.build_harness()
    real = make(0)
    assert np.array_equal(got["labels"].cpu().numpy(), kc.harness_dbscan(h, real["points"])[0])
    assert np.array_equal(got["select_status"].cpu().numpy(), kc.harness_select(h, real["means"], real["scores"])["words"])


# ---- select_target ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _select_case(kind="map"):
    means, scores, _ = kc.qualifying_select_case(kind=kind)
    want = kc.restate_select(means, scores)
    for a in (means, scores):
        a.setflags(write=False)
    return means, scores, want


def _check_selection(sel, want):
    got = dict(band_idx=sel.points_index_range, above_idx=sel.points_index, labels=sel.labels, selected_idx=sel.selected_points_index)
    for k, v in got.items():
        assert v.is_cuda and v.dtype == torch.int32 and np.array_equal(v.cpu().numpy(), want[k]), k
    assert sel.threshold.cpu().numpy().view(np.uint32) == np.asarray(want["threshold"]).view(np.uint32)
    assert (sel.n_band, sel.n_above, sel.n_clusters, sel.max_label, sel.n_selected, sel.argmax) == \
           (len(want["band_idx"]), len(want["above_idx"]), want["n_clusters"], want["max_label"], len(want["selected_idx"]), want["argmax"])


def test_select_target_equals_the_torch_chain_and_the_harness(gpu):
    from fisher_rast.cluster import select_target
    means, scores, want = _select_case()
    sel = select_target(torch.from_numpy(np.array(means)).to(gpu), torch.from_numpy(np.array(scores)).to(gpu), kc.LOWER_Y, kc.UPPER_Y)
    _check_selection(sel, want)
    assert sel.n_clusters >= 2 and 0 < sel.n_selected < sel.n_above and not sel.nan_scores
    hs = kc.harness_select(kc.build_harness(), means, scores)["status"]
    assert np.array_equal(np.array(sel.cell_sides, F), hs["sides"])
    _check_selection(select_target(means, scores.astype(np.float64), kc.LOWER_Y, kc.UPPER_Y), want)      # NumPy in, float64 scores


def test_select_target_reads_the_host_once(gpu):
    from fisher_rast.cluster import select_target
    means, scores, want = _select_case()
    m, s = torch.from_numpy(np.array(means)).to(gpu), torch.from_numpy(np.array(scores)).to(gpu)
    select_target(m, s, kc.LOWER_Y, kc.UPPER_Y)                      # (allocator warm)
    torch.cuda.synchronize()
    reads = []
    orig = torch.Tensor.cpu

    def counting(self, *a, **k):
        reads.append(tuple(self.shape))
        return orig(self, *a, **k)
    torch.Tensor.cpu = counting
    try:
        torch.cuda.set_sync_debug_mode("warn")
        import warnings
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            sel = select_target(m, s, kc.LOWER_Y, kc.UPPER_Y)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        torch.Tensor.cpu = orig
    assert reads == [(16,)] and len([x for x in w if "synchroniz" in str(x.message)]) == 1, (reads, [str(x.message) for x in w])
    assert sel.n_above == len(want["above_idx"])


def test_select_target_edges(gpu):
    from fisher_rast.cluster import select_target
    means, scores, want = _select_case("equal")
    m = torch.from_numpy(np.array(means)).to(gpu)
    sel = select_target(m, torch.from_numpy(np.array(scores)).to(gpu), kc.LOWER_Y, kc.UPPER_Y)
    _check_selection(sel, want)                                       # every score equal: the reference's `else` branch
    assert sel.n_above == 0 and sel.argmax == int(want["band_idx"][0]) and sel.max_label == -1
    with pytest.raises(RuntimeError, match="non-empty"):
        select_target(m, torch.from_numpy(np.array(scores)).to(gpu), 50.0, 60.0)
    bad = np.array(_select_case()[1])
    row = int(_select_case()[2]["band_idx"][3])
    bad[row] = np.nan
    sel = select_target(torch.from_numpy(np.array(_select_case()[0])).to(gpu), torch.from_numpy(bad).to(gpu), kc.LOWER_Y, kc.UPPER_Y)
    assert sel.nan_scores and sel.n_above == 0 and sel.argmax == row and bool(torch.isnan(sel.threshold))      # the torch route
    assert np.array_equal(sel.points_index_range.cpu().numpy(), _select_case()[2]["band_idx"])
    # no cluster qualifies: max_label stays -1 and the NOISE rows are the selected ones
    sparse = np.stack([np.arange(40) * 1.0, np.zeros(40), np.zeros(40)], 1).astype(F)
    sel = select_target(sparse, np.arange(40, dtype=F), -1.0, 1.0)
    assert sel.n_clusters == 0 and sel.max_label == -1 and sel.n_selected == sel.n_above == 8
    assert sel.selected_points_index.cpu().numpy().tolist() == list(range(32, 40))


# ---- global_planning ------------------------------------------------------------------------------------------------------------------

PLAN_P, PLAN_W, PLAN_K = 8000, 128, 10
REJECTED, RAISES = (1, 4), 6


class _Pathfinder:
    def __init__(self, positions, agent_y):
        self.positions, self.agent_y, self.asked = positions, agent_y, []

    def index_of(self, pos):
        return int(np.argmin(np.abs(self.positions[:, [0, 2]] - np.asarray(pos)[[0, 2]]).sum(1)))

    def is_navigable(self, pos):
        assert pos[1] == self.agent_y                                 # the candidate's height is replaced by the agent's
        self.asked.append(self.index_of(pos))
        return self.asked[-1] not in REJECTED


class _Follower:
    def __init__(self, positions, agent_y):
        self.pathfinder, self.resets = _Pathfinder(positions, agent_y), 0

    def reset(self):
        self.resets += 1

    def find_path(self, pos):
        if self.pathfinder.index_of(pos) == RAISES:
            raise RuntimeError("the follower fails on a navigable point")
        return iter([1, 2, 3])


def _planning_slam(gpu, seed):
    from fisher_rast import synthetic
    from models.SLAM.gaussian import GaussianSLAM, TargetSelectOps

    class Slam(GaussianSLAM):
        def build_frontiers(self):
            return None

        def generate_Gaussian_at_frontier(self):
            self.frontier_calls = getattr(self, "frontier_calls", 0) + 1

        def generate_candidate(self, center_point):
            self.center_point = center_point
            return self.candidates
    TargetSelectOps.install(Slam)
    params = synthetic.room_shell(PLAN_P, seed=seed)
    means, _ = kc.make_select_case(PLAN_P, seed=seed)
    params["means3D"] = torch.from_numpy(means)
    slam = Slam(params=params, intrinsics=synthetic.intrinsics(PLAN_W, PLAN_W), width=PLAN_W, height=PLAN_W, device=gpu)
    slam.config = {"explore": {"height_range": 0.3, "sample_view_num": PLAN_K, "prune_invisible": True}}
    slam.cam_height, slam.selection = 0.0, 2
    for w in synthetic.invert_rigid(synthetic.candidate_poses(16, seed=seed + 50)):
        slam.add_keyframe(w.to(gpu))
    slam.candidates = synthetic.candidate_poses(PLAN_K, seed=seed + 70).to(gpu)
    slam.variables = {k: torch.arange(PLAN_P, dtype=torch.float32, device=gpu) + i for i, k in
                      enumerate(("max_2D_radius", "means2D_gradient_accum", "denom", "timestep"))}
    return slam


def test_global_planning_against_a_per_view_loop(gpu):
    from scenes import rel_err
    from models.SLAM.gaussian import GaussianSLAM
    assert not hasattr(GaussianSLAM, "global_planning")              # opt-in: the product class itself is untouched
    slam = _planning_slam(gpu, seed=0)
    means0 = slam.params["means3D"].clone()
    agent_pose = np.eye(4)
    agent_pose[1, 3] = 0.25
    follower = _Follower(slam.candidates[:, :3, 3].cpu().numpy(), 0.25)

    # the restatement: gaussian.py:1188-1198 and 1285-1316 as loops over per-view compute_Hessian
    H_train = sum(slam.compute_Hessian(kf["est_w2c"], return_points=True) for kf in slam.keyframe_list)
    H_inv = torch.reciprocal(H_train + 0.1)
    score_ref = H_inv.sum(1)
    survivors = [i for i in range(PLAN_K) if i not in REJECTED and i != RAISES]
    max_ref = torch.zeros((PLAN_P,), device=gpu)
    view_ref = []
    for i in survivors:
        cur_H = slam.compute_Hessian(torch.linalg.inv(slam.candidates[i]), return_points=True)
        ps = (cur_H * H_inv).sum(1)
        max_ref = torch.where(max_ref > ps, max_ref, ps)
        view_ref.append(float((cur_H * H_inv).sum()))
    seen = {}
    orig = slam.select_target_points

    def recording(scorePoints, K, **kw):
        seen["scores"] = scorePoints.clone()
        np.random.seed(11)
        seen["out"] = orig(scorePoints, K, **kw)
        return seen["out"]
    slam.select_target_points = recording
    scores, c2ws = slam.global_planning(follower, agent_pose)

    # the scores global_planning selected on are the per-view loop's within the bar of pose_eval
    assert rel_err(seen["scores"].cpu().numpy(), score_ref.cpu().numpy()) < 1e-4
    # the selection on those scores: every list equal to the torch + restatement chain, the draw the seeded reference draw
    sp = seen["scores"].cpu().numpy()
    want = kc.restate_select(means0.cpu().numpy(), sp, -0.3, 0.3)
    assert kc.qualifies(means0.cpu().numpy()[want["above_idx"]])
    assert len(want["selected_idx"]) > 0 and want["max_label"] >= 0, (len(want["above_idx"]), want["n_clusters"])
    centre, selected = seen["out"]
    assert selected.dtype == torch.int64 and np.array_equal(selected.cpu().numpy(), want["selected_idx"])
    np.random.seed(11)
    draws = np.random.randint(0, len(want["selected_idx"]), (PLAN_K,))
    assert torch.equal(centre, means0[torch.from_numpy(want["selected_idx"][draws].astype(np.int64)).to(gpu)]) and slam.center_point is centre
    # the follower: every candidate asked in order, two rejected, one raises and is skipped
    assert follower.pathfinder.asked == list(range(PLAN_K)) and follower.resets == PLAN_K - len(REJECTED)
    assert torch.equal(c2ws, slam.candidates[survivors]) and scores.shape == (len(survivors),) and scores.device.type == "cpu"
    assert rel_err(scores.numpy(), np.array(view_ref, F)) < 1e-4
    # the prune rule on a case where no selected point lies within the score tolerance of the 2 x rule (checked here)
    sel = torch.from_numpy(want["selected_idx"].astype(np.int64)).to(gpu)
    twice = score_ref[sel] * 2
    gap = (max_ref[sel] - twice).abs()
    assert bool((gap > 1e-3 * torch.maximum(twice, max_ref[sel]) + 1e-7 * max_ref.max()).all()), float(gap.min())
    remove = torch.zeros((PLAN_P,), dtype=torch.bool, device=gpu)
    remove[sel[max_ref[sel] < twice]] = True
    assert 0 < int(remove.sum()) and slam.params["means3D"].shape[0] == PLAN_P - int(remove.sum())
    assert torch.equal(slam.params["means3D"], means0[~remove]) and torch.equal(slam.variables["denom"], (torch.arange(PLAN_P, device=gpu) + 2.0)[~remove])
    assert slam.selection == 3 and slam.frontier_calls == 1


def test_global_planning_when_nothing_is_navigable_and_on_the_frontier_branch(gpu):
    slam = _planning_slam(gpu, seed=0)
    follower = _Follower(slam.candidates[:, :3, 3].cpu().numpy(), 0.0)
    follower.pathfinder.is_navigable = lambda pos: False
    P0 = slam.params["means3D"].shape[0]
    assert slam.global_planning(follower, np.eye(4)) == (None, None) and slam.selection == 3
    assert slam.params["means3D"].shape[0] < P0                      # max_points_score stayed zero: every selected point is pruned, as in the reference
    # a frontier while selection < 2: the centres are frontier cells at the camera height, nothing is selected or pruned
    slam = _planning_slam(gpu, seed=0)
    slam.selection = 0
    slam.build_frontiers = lambda: np.array([[1.0, 2.0], [-3.0, 0.5]])
    scores, c2ws = slam.global_planning(_Follower(slam.candidates[:, :3, 3].cpu().numpy(), 0.0), np.eye(4))
    cp = slam.center_point.cpu().numpy()
    assert cp.shape == (PLAN_K, 3) and (cp[:, 1] == 0.0).all() and set(map(tuple, cp[:, [0, 2]])) <= {(1.0, 2.0), (-3.0, 0.5)}
    assert slam.params["means3D"].shape[0] == PLAN_P and scores.shape[0] == c2ws.shape[0] == PLAN_K - len(REJECTED) - 1 and slam.selection == 1
