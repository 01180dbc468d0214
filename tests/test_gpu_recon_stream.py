"""-m gpu: the running reconstruction metrics on the device.  The seeded search (CloudIndex.fold) against the plain search of the union
BIT FOR BIT; seeds that decide; the masked depth source against a zeroed depth image; out_points against the g++ harness; the
ReconTracker against reconstruction_metrics on the concatenated frames and against the SciPy float64 statement; host
synchronisations counted; stream order by the procedure of tests/stream_cases.py; ReconStreamOps.install on a stub class."""
import functools
import warnings

import numpy as np
import pytest
import torch

import cloud_cases as cc
import recon_cases as rc
import stream_cases as sc

pytestmark = pytest.mark.gpu

TH = 0.05
INF = float("inf")


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8).reshape(-1).tobytes()


def _same(got, want, what):
    assert tuple(got.shape) == tuple(want.shape) and _bits(got) == _bits(want), what


def _host_sqrt(seed):
    return np.sqrt(seed.cpu().numpy())                        # (IEEE on the host, as frc_distance on the device)


# ---- 1. fold equals the union ---------------------------------------------------------------------------------------------------------

def _fold_all(frames, q, gpu, CloudIndex):
    seed = torch.full((q.shape[0],), INF, device=gpu)
    r = None
    for f in frames:
        r = CloudIndex(_dev(f, gpu)).fold(q, seed, TH, dist=True, flag=True, stats=True)
    return seed, r


@pytest.mark.parametrize("family", rc.FOLD_FAMILIES)
def test_fold_equals_the_union_bit_for_bit(gpu, family):
    """seeds +inf, folded frame by frame: sqrt of the seeds, the last fold's distances, flags and statistics are those of ONE search
    against the concatenation, on every byte; the reversed order gives the same bytes; folding the last frame again changes nothing"""
    from fisher_rast.cloud import CloudIndex
    for N in rc.FOLD_N:
        for M in rc.FOLD_M:
            t, q, _ = cc.qualifying_case(family, N, M)
            qd = _dev(q, gpu)
            for k in rc.FOLD_K:
                frames = rc.cut(t, k)
                union = CloudIndex(_dev(np.concatenate(frames), gpu))
                want = union.search(qd, TH, dist=True, flag=True, stats=True)
                what = (family, N, M, k)
                seed, r = _fold_all(frames, qd, gpu, CloudIndex)
                _same(_host_sqrt(seed), want["dist"], (what, "sqrt of the seeds"))
                for n in ("dist", "flag", "stats"):
                    _same(r[n], want[n], (what, n))
                seed_rev, r_rev = _fold_all(frames[::-1], qd, gpu, CloudIndex)
                _same(seed_rev, seed, (what, "reversed order"))
                _same(r_rev["stats"], want["stats"], (what, "reversed order, stats"))
                again = CloudIndex(_dev(frames[-1], gpu)).fold(qd, seed_rev, TH, dist=True, flag=True, stats=True)
                _same(seed_rev, seed, (what, "the last frame a second time"))
                for n in ("dist", "flag", "stats"):
                    _same(again[n], want[n], (what, n, "second time"))


# ---- 2. seeds that decide -------------------------------------------------------------------------------------------------------------

def test_seeds_that_decide(gpu):
    """65 queries against 1025 targets, so that one wave holds live and dead lanes: a seed of 0 stays 0, a seed equal to the exact
    squared distance stays with its bits, one ulp above it is replaced, +inf is replaced; a non-finite query keeps its seed and is
    counted as skipped"""
    from fisher_rast.cloud import CloudIndex, decode_stats
    t, q, _ = cc.qualifying_case("uniform", 1025, 65)
    q = q.copy()
    q[37, 1] = np.nan
    exact = rc.harness_fold(rc.build_harness(), t, q, np.full(65, np.inf, np.float32))
    assert np.isfinite(np.delete(exact, 37)).all() and (np.delete(exact, 37) > 0).all() and np.isinf(exact[37])
    i = np.arange(65)
    seed = np.where(i % 4 == 0, np.float32(0), np.where(i % 4 == 1, exact, np.where(i % 4 == 2, np.nextafter(exact, np.float32(np.inf)), np.float32(np.inf))))
    seed = seed.astype(np.float32)
    seed[37] = 7.0
    want = np.where(i % 4 == 0, np.float32(0), exact).astype(np.float32)
    want[37] = 7.0
    sd = _dev(seed, gpu)
    r = CloudIndex(_dev(t, gpu)).fold(_dev(q, gpu), sd, TH, dist=True, flag=True, stats=True)
    _same(sd, want, "seeds")
    ok = i != 37
    _same(r["dist"][torch.from_numpy(ok).to(gpu)], np.sqrt(want[ok]), "dist")
    assert float(r["dist"][37]) == INF and int(r["flag"][37]) == 0
    s = decode_stats(r["stats"].cpu().numpy())
    assert s["valid"] == 64 and s["skipped"] == 1 and s["flagged"] == int((np.sqrt(want[ok]) < np.float32(TH)).sum()) == int(r["flag"].sum())
    # whatever the targets are: an index without a target, and one whose every target coincides with a query
    for targets in (torch.zeros((0, 3), device=gpu), _dev(q[ok], gpu)):
        zero = torch.zeros((65,), device=gpu)
        CloudIndex(targets).fold(_dev(q, gpu), zero, TH)
        assert _bits(zero) == bytes(65 * 4)


# ---- 3. the mask ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", cc.DEPTH_SHAPES)
@pytest.mark.parametrize("kind", ["object", "few"])
def test_mask_equals_a_zeroed_depth(gpu, H, W, kind):
    from fisher_rast.cloud import CloudIndex, decode_stats
    c = cc.qualifying_depth_case(H, W, kind, "-Z")
    rng = np.random.default_rng([H, W, kind == "few"])
    pm = (rng.uniform(size=(H, W)) < 0.6).astype(np.uint8) * rng.integers(1, 256, (H, W)).astype(np.uint8)       # any non-zero byte is "in"
    pm[8:20, 14:30] = 255                                      # the object of both kinds lies inside
    pm[24:32, 0:8] = 0                                         # an 8 x 8 block of the grid fully masked out
    zeroed = c["depth"].copy()
    zeroed[pm == 0] = 0.0
    ix = CloudIndex(_dev(c["env"], gpu))
    depth, depth0, pmd, kinv, c2w = _dev(c["depth"], gpu), _dev(zeroed, gpu), _dev(pm, gpu), cc.depth_kinv(c), _dev(c["c2w"], gpu)
    none_valid = cc.qualifying_depth_case(H, W, "none-valid", "-Z")
    for stride in (1, 2, 3):
        want = ix.query_depth(depth0, kinv, c2w, stride=stride, flip_z=True, dist_th=TH, want_dist=True)
        got = ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=True, dist_th=TH, want_dist=True, mask=pmd)
        for g, w, n in zip(got, want, ("mask", "stats", "dist")):
            _same(g, w, (kind, stride, n))
        assert decode_stats(got[1].cpu().numpy())["valid"] > 0
        # a bool mask is the same mask
        _same(ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=True, dist_th=TH, mask=pmd > 0)[1], want[1], (kind, stride, "bool mask"))
        # near: d < th, counted from the distances
        flag, stats, dist = ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=True, dist_th=TH, want_dist=True, mask=pmd, near=True)
        _same(dist, want[2], (kind, stride, "near dist"))
        d = dist.cpu().numpy()
        s, s_novel = decode_stats(stats.cpu().numpy()), decode_stats(want[1].cpu().numpy())
        assert s["flagged"] == int((d < np.float32(TH)).sum()) and np.array_equal(flag.cpu().numpy().astype(bool), d < np.float32(TH))
        assert (s["sum"], s["valid"], s["skipped"]) == (s_novel["sum"], s_novel["valid"], s_novel["skipped"]) and 0 < s["flagged"] < s["valid"]
        # a mask of all zeros: the statistics of an image without any depth
        empty = ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=True, dist_th=TH, want_dist=True, mask=torch.zeros_like(pmd))
        nv = ix.query_depth(_dev(none_valid["depth"], gpu), cc.depth_kinv(none_valid), _dev(none_valid["c2w"], gpu), stride=stride, flip_z=True, dist_th=TH)
        _same(empty[1], nv[1], (kind, stride, "all-zero mask"))
        assert not empty[0].any() and torch.isinf(empty[2]).all()


# ---- 4. out_points --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("H,W", cc.DEPTH_SHAPES)
def test_out_points(gpu, H, W):
    """every valid sample equals the harness's frc_back_project on every byte, every other row is three NaNs, and an index built
    over the array as it stands answers as an index over its finite rows"""
    from fisher_rast.cloud import CloudIndex
    h = rc.build_harness()
    c = cc.qualifying_depth_case(H, W, "object", "-Z")
    pm = (np.random.default_rng(4).uniform(size=(H, W)) < 0.7).astype(np.uint8)
    ix = CloudIndex(_dev(c["env"], gpu))
    kinv = cc.depth_kinv(c)
    _, q, _ = cc.qualifying_case("uniform", 1025, 257)
    qd = _dev(q / 2, gpu)
    for stride in (1, 2, 3):
        for mask in (None, pm):
            want, valid = rc.harness_points(h, c["depth"], mask, kinv, c["c2w"], stride, True)
            r = ix.query_depth(_dev(c["depth"], gpu), kinv, _dev(c["c2w"], gpu), stride=stride, flip_z=True, dist_th=TH,
                               mask=None if mask is None else _dev(mask, gpu), want_points=True)
            assert len(r) == 3
            pts = r[2]
            got = pts.cpu().numpy()
            assert got.shape == want.shape and 0 < valid.sum() < len(valid)
            assert _bits(got[valid]) == _bits(want[valid]), (stride, mask is None)
            assert np.isnan(got[~valid]).all()
            _same(CloudIndex(pts).query(qd), CloudIndex(_dev(want[valid], gpu)).query(qd), (stride, "index over out_points"))
            # the points alone, no other output asked for by the caller of the ABI: the same bytes with want_dist
            r4 = ix.query_depth(_dev(c["depth"], gpu), kinv, _dev(c["c2w"], gpu), stride=stride, flip_z=True, dist_th=TH,
                                mask=None if mask is None else _dev(mask, gpu), want_dist=True, want_points=True)
            assert len(r4) == 4 and _bits(r4[3]) == _bits(pts)


# ---- 5. and 6. the tracker --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _scene(n_gt):
    h = rc.build_harness()
    s = rc.qualifying_scene(h, n_gt)
    upto = [rc.scene_points(h, s, k) for k in range(len(s["frames"]) + 1)]
    for a in upto:
        a.setflags(write=False)
    return s, upto


def _add(tracker, s, fr, gpu, **kw):
    kinv, T = rc.frame_transform(s, fr)
    tracker.add_frame(_dev(fr["depth"], gpu), kinv, T, mask=_dev(fr["mask"], gpu), **kw)


def _eq(a, b):
    return a == b or (a != a and b != b)


@pytest.mark.parametrize("n_gt", [1000, 5000])
@pytest.mark.parametrize("th", cc.THRESHOLDS)
def test_tracker_against_the_batch_route(gpu, n_gt, th):
    """after every frame, and before the first: comp, ratio, iratio, fpr and n_rec equal exactly; acc within relative 2 n 2^-53 (both
    are binary64 sums of the same n non-negative binary32 distances in different groupings, each within n 2^-53 of the exact sum)"""
    from fisher_rast.cloud import CloudIndex, ReconTracker, reconstruction_metrics
    s, upto = _scene(n_gt)
    gt = CloudIndex(_dev(s["gt"], gpu))
    tracker = ReconTracker(gt, th)
    for k in range(len(s["frames"]) + 1):
        if k:
            _add(tracker, s, s["frames"][k - 1], gpu)
        got, want = tracker.metrics(), reconstruction_metrics(gt, _dev(upto[k], gpu), th)
        print(f"n_gt {n_gt} th {th} frame {k}: {got}")
        assert got["n_rec"] == len(upto[k]) and set(got) == set(want) | {"n_rec"}
        for n in ("comp", "ratio", "iratio", "fpr"):
            assert _eq(got[n], want[n]), (k, n, got, want)
        if k:
            assert abs(got["acc"] - want["acc"]) <= 2 * got["n_rec"] * 2.0 ** -53 * abs(want["acc"]), (k, got, want)
            assert 0 < got["ratio"] <= 1 and 0 < got["iratio"] < 1 and got["comp"] > 0
        else:
            assert got["acc"] != got["acc"] and got["comp"] == INF and got["ratio"] == 0.0
    # metrics() changes nothing; add_points of the same frames gives the same numbers; reset() is the initial state
    assert tracker.metrics() == got
    other = ReconTracker(gt, th, keep_points=True)
    for k in range(len(s["frames"])):
        other.add_points(upto[k + 1][len(upto[k]):])
    m = other.metrics()
    assert all(_eq(m[n], got[n]) for n in ("comp", "ratio", "iratio", "fpr", "n_rec")) and abs(m["acc"] - got["acc"]) <= 2 * m["n_rec"] * 2.0 ** -53 * got["acc"]
    _same(other.cloud(), upto[-1], "cloud()")
    first = ReconTracker(gt, th).metrics()
    tracker.reset()
    again = tracker.metrics()
    assert all(_eq(again[n], first[n]) for n in first) and again["n_rec"] == 0 and torch.isinf(tracker.best_d2).all()


@pytest.mark.parametrize("n_gt", [1000, 5000])
def test_tracker_against_the_float64_statement(gpu, n_gt):
    """acc and comp to relative 1e-6 (the unit's contract), ratio exactly, on a scene that qualifies for both thresholds"""
    from fisher_rast.cloud import ReconTracker
    s, upto = _scene(n_gt)
    assert all(cc.qualifies_points(s["gt"], upto[k]) and cc.qualifies_points(upto[k], s["gt"]) for k in range(1, len(upto)))
    for th in cc.THRESHOLDS:
        tracker = ReconTracker(_dev(s["gt"], gpu), th)
        for k, fr in enumerate(s["frames"], 1):
            _add(tracker, s, fr, gpu)
            if k in (1, len(s["frames"])):
                got = tracker.metrics()
                acc, comp, ratio = cc.scipy_metrics(s["gt"], upto[k], th)
                assert abs(got["acc"] - acc) <= 1e-6 * acc and abs(got["comp"] - comp) <= 1e-6 * comp and got["ratio"] == ratio, (th, k, got, (acc, comp, ratio))
                iratio = float(np.mean((cc.scipy_nearest(s["gt"], upto[k])[0] < th).astype(float)))
                assert got["iratio"] == iratio and got["fpr"] == 1.0 - iratio


# ---- 7. host synchronisations -----------------------------------------------------------------------------------------------------------

def _syncs(fn):
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, [x for x in w if "synchroniz" in str(x.message).lower() and "prototype" not in str(x.message).lower()]


def test_host_synchronisations(gpu):
    """none in add_frame and add_points (nor in fold and the masked query_depth under them); exactly one host read in metrics()"""
    from fisher_rast.cloud import ReconTracker
    s, upto = _scene(1000)
    tracker = ReconTracker(_dev(s["gt"], gpu), TH, keep_points=True)
    frames = [(_dev(fr["depth"], gpu), *rc.frame_transform(s, fr), _dev(fr["mask"], gpu)) for fr in s["frames"]]
    pts = _dev(upto[1], gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for depth, kinv, T, mask in frames[:3]:
            tracker.add_frame(depth, kinv, T, mask=mask)
        tracker.add_frame(frames[3][0], frames[3][1], frames[3][2], stride=2)
        tracker.add_points(pts)
        tracker.add_points(upto[1])                             # a host cloud: staged, not waited for
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    m, syncs = _syncs(tracker.metrics)
    print(f"metrics(): host synchronisations {len(syncs)}")
    assert len(syncs) == 1, [str(x.message) for x in syncs]
    assert m["n_rec"] > 3 * len(upto[1]) and 0 < m["ratio"] <= 1


# ---- 8. stream order ------------------------------------------------------------------------------------------------------------------

def test_add_frame_in_stream_order(gpu):
    """add_frame and the device-side statistics on a caller stream, behind a blocker and against a decoy of the same shape, twice
    back to back: tests/stream_cases.py's procedure.  The case lives here; the table and its counts are not touched."""
    def make(which):
        s = rc.make_scene(1000, n_frames=1, seed=20 + which)
        fr = s["frames"][0]
        kinv, T = rc.frame_transform(s, fr)
        return dict(gt=s["gt"], depth=np.nan_to_num(fr["depth"], nan=0.0, posinf=0.0), mask=(fr["mask"] > 0).astype(np.uint8), kinv=kinv,
                    cam_to_eval=np.ascontiguousarray(T[:3]))

    def call(ctx, b):
        from fisher_rast.cloud import ReconTracker
        tracker = ReconTracker(b["gt"], TH)
        tracker.add_frame(b["depth"], b["kinv"], b["cam_to_eval"], mask=b["mask"])
        comp = tracker._empty.fold(tracker.gt.points, tracker.best_d2, TH, stats=True)["stats"]
        return dict(best_d2=tracker.best_d2, running=tracker.running, completion=comp)

    case = sc.Case(name="recon_tracker_add_frame", make=make, call=call, exact=("best_d2", "running", "completion"), same=("kinv",),
                   sync_free=True, repeat=True, covers=("fr_cloud_index_build", "fr_cloud_query"))
    ref, got = sc.run_case(case, gpu, check_covers=True)
    # and the stream-ordered run is the real frame's result, stated without the tracker
    from fisher_rast.cloud import decode_stats
    real = make(0)
    h = rc.build_harness()
    pts, valid = rc.harness_points(h, real["depth"], real["mask"], real["kinv"], real["cam_to_eval"])
    want = rc.harness_fold(h, pts[valid], real["gt"], np.full(len(real["gt"]), np.inf, np.float32))
    _same(got["best_d2"], want, "best_d2 of the stream-ordered run")
    assert decode_stats(got["running"].cpu().numpy())["valid"] == int(valid.sum())
    print(f"enqueue {sc.ENQUEUE_MS[case.name]:.3f} ms behind a blocker of {sc.BLOCKER_MS} ms")


# ---- 9. the reference's call sites ------------------------------------------------------------------------------------------------------

def test_install_on_a_stub_class(gpu, tmp_path):
    import yaml
    from fisher_rast import cloud
    s, upto = _scene(1000)

    class Tester:
        def __init__(self):
            self.gt_obj_3d_rotated = torch.from_numpy(np.array(s["gt"]))
            self.policy_eval_dir = str(tmp_path)
            self.policy_name = "stub"

        def store_filtered_obj_pointcloud(self, *a, **k):
            raise AssertionError("the reference's method was left in place")

        def evaluate_3d_object_reconstruction(self, step=0):
            raise AssertionError("the reference's method was left in place")

    assert cloud.ReconStreamOps.install(Tester, eval_transform=s["eval_transform"], dist_th=0.01) is Tester
    t = Tester()
    rgb = np.zeros((48, 64, 3), np.uint8)
    for step, fr in enumerate(s["frames"][:3]):
        assert t.store_filtered_obj_pointcloud(rgb, fr["depth"], torch.from_numpy(fr["intrinsics"]), fr["mask"], fr["camera_pose"], fr["object_pose"], step=step) is None
    # an empty mask: None, and nothing is added
    assert t.store_filtered_obj_pointcloud(rgb, s["frames"][3]["depth"], s["frames"][3]["intrinsics"], np.zeros((48, 64), np.uint8),
                                           s["frames"][3]["camera_pose"], s["frames"][3]["object_pose"], step=3) is None
    assert t.recon_tracker.frames == 3
    t.evaluate_3d_object_reconstruction(step=2)
    m = t.recon_tracker.metrics()
    assert m["n_rec"] == len(upto[3])
    want = cloud.reconstruction_metrics(t.recon_tracker.gt, _dev(upto[3], gpu), 0.01)
    assert all(_eq(m[n], want[n]) for n in ("comp", "ratio", "iratio", "fpr"))
    with open(tmp_path / "metrics" / "object_recon_metrics.yaml") as f:
        data = yaml.safe_load(f)
    assert len(data["steps"]) == 1 and data["experiment"]["policy_name"] == "stub" and data["settings"]["distance_threshold_m"] == 0.01
    row = data["steps"][0]
    assert row["step"] == 2 and [row[k] for k in ("acc_distance_m", "comp_distance_m", "completeness_ratio", "fpr")] == \
        [m["acc"] * 100, m["comp"] * 100, m["ratio"] * 100, m["fpr"] * 100]
    assert data["summary"]["last_step"] == 2 and data["summary"]["last_completeness_percent"] == m["ratio"] * 100
    t.evaluate_3d_object_reconstruction(step=5)
    with open(tmp_path / "metrics" / "object_recon_metrics.yaml") as f:
        assert [r["step"] for r in yaml.safe_load(f)["steps"]] == [2, 5]
