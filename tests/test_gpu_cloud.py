"""-m gpu: the nearest-point search on the device (csrc/fr_cloud.hip through fisher_rast/cloud.py) against the g++ harness over the
same header (tests/harness/fr_cloud_harness.cpp) BIT FOR BIT -- distances, lowest-index ties, flags, the statistics' binary64 sum --
at every family and size of tests/cloud_cases.py (wave, sub-box, box and sort-chunk edges), all outputs on and each alone; the depth
mode; the drop-ins against the outputs of the reference's own functions (tests/golden/reference_cloud.npz); index reuse; host
synchronisations counted; one run on a non-default stream by the procedure of tests/stream_cases.py."""
import functools
import os
import warnings

import numpy as np
import pytest
import torch

import cloud_cases as cc
import stream_cases as sc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cloud.npz")
TH = 0.05


@pytest.fixture(scope="module")
def cloud_harness():
    return cc.build_harness()


@functools.lru_cache(maxsize=None)
def _case(family, N, M):
    """the case and the harness's statement of it, computed once and shared (read-only)"""
    t, q, _ = cc.qualifying_case(family, N, M)
    want = cc.harness_query(cc.build_harness(), t, q, TH)
    for a in (t, q, *want.values()):
        a.setflags(write=False)
    return t, q, want


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)             # (a copy: the shared cases are read-only)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint8).reshape(-1).tobytes()


def _same(got, want, what):
    assert tuple(got.shape) == tuple(want.shape) and _bits(got) == _bits(want), what


def _check(r, want, what, names=("dist", "index", "flag", "stats")):
    key = dict(dist="dist", index="idx", flag="flag", stats="stats")
    for n in names:
        _same(r[n], want[key[n]], (what, n))


SUPER = 16 * 1024                      # targets per top-level box of the index (csrc/fr_cloud.hip: FRC_SUPER boxes of FRC_BOX points)
SIZES = [(N, M) for N in cc.N_SIZES for M in cc.M_SIZES] + [(SUPER, 257), (SUPER + 1, 257), (cc.N_LARGE, 1000)]


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_search_equals_the_harness_bit_for_bit(gpu, family):
    """out_dist, out_idx, out_flag and the statistics at every size, all outputs on and each alone"""
    from fisher_rast.cloud import CloudIndex
    for N, M in SIZES:
        t, q, want = _case(family, N, M)
        ix = CloudIndex(_dev(t, gpu))
        qd = _dev(q, gpu)
        _check(ix.search(qd, TH, dist=True, index=True, flag=True, stats=True), want, (family, N, M))
        for alone in ("dist", "index", "flag", "stats"):
            r = ix.search(qd, TH, **{k: k == alone for k in ("dist", "index", "flag", "stats")})
            assert all(r[k] is None for k in r if k != alone)
            _check(r, want, (family, N, M, "alone"), names=(alone,))


@pytest.mark.parametrize("family", ["clusters", "outside", "nonfinite"])
def test_result_does_not_depend_on_the_order_of_the_queries(gpu, family):
    """a permuted query set gives the permuted result (ties and duplicates included); the counts are those of the harness"""
    from fisher_rast.cloud import CloudIndex
    t, q, want = _case(family, 2049, 1000)
    ix = CloudIndex(_dev(t, gpu))
    perm = np.random.default_rng(3).permutation(len(q))
    r = ix.search(_dev(q[perm], gpu), TH, index=True, flag=True, stats=True)
    _same(r["dist"], want["dist"][perm], "dist")
    _same(r["index"], want["idx"][perm], "index")
    _same(r["flag"], want["flag"][perm], "flag")
    assert r["stats"].cpu().numpy()[1:].tolist() == want["stats"][1:].astype(np.int64).tolist()


def test_statistics_are_reproducible(gpu):
    """two runs of the same call give identical bytes, and the bytes are the harness's (fixed order of binary64 sums)"""
    from fisher_rast.cloud import CloudIndex, decode_stats
    t, q, want = _case("surface", cc.N_LARGE, 1000)
    ix = CloudIndex(_dev(t, gpu))
    qd = _dev(q, gpu)
    a, b = ix.stats(qd, TH), ix.stats(qd, TH)
    assert _bits(a) == _bits(b) == _bits(want["stats"])
    assert decode_stats(a.cpu().numpy()) == cc.decode(want["stats"])
    # many partials: the caller order decides the sum, so a large query set against a small index is checked as well
    rng = np.random.default_rng(9)
    big = rng.uniform(-4, 4, (70001, 3)).astype(np.float32)
    tt = rng.uniform(-4, 4, (65, 3)).astype(np.float32)
    w = cc.harness_query(cc.build_harness(), tt, big, TH)
    r = CloudIndex(_dev(tt, gpu)).search(_dev(big, gpu), TH, index=True, stats=True)
    _check(r, w, "70001 queries", names=("dist", "index", "stats"))


@pytest.mark.parametrize("H,W", cc.DEPTH_SHAPES)
@pytest.mark.parametrize("z_forward", ["-Z", "Z"])
def test_depth_mode_equals_the_harness(gpu, cloud_harness, H, W, z_forward):
    """mask, statistics and the generated points' distances bit for bit, strides 1, 2, 3; the last pixel is valid (the edge of the last
    wave's block), and at stride 1 one 8 x 8 block of the grid has no valid pixel at all"""
    from fisher_rast.cloud import CloudIndex
    for kind in cc.DEPTH_KINDS:
        c = cc.qualifying_depth_case(H, W, kind, z_forward)
        ix = CloudIndex(_dev(c["env"], gpu))
        depth, kinv, c2w = _dev(c["depth"], gpu), cc.depth_kinv(c), _dev(c["c2w"], gpu)
        for stride in (1, 2, 3):
            want = cc.harness_depth(cloud_harness, c, stride)
            mask, stats, dist = ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=z_forward == "-Z", dist_th=TH, want_dist=True)
            _same(mask, want["flag"], (kind, stride, "mask"))
            _same(dist, want["dist"], (kind, stride, "dist"))
            _same(stats, want["stats"], (kind, stride, "stats"))
            mask2, stats2 = ix.query_depth(depth, kinv, c2w, stride=stride, flip_z=z_forward == "-Z", dist_th=TH)
            assert _bits(mask2) == _bits(mask) and _bits(stats2) == _bits(stats)
            if kind != "none-valid" and stride == 1:               # (at stride 3 the last sample is not the last pixel)
                assert want["valid"][-1, -1] == 1 and np.isfinite(want["dist"][-1, -1])
                assert not want["valid"][16:24, 8:16].any() and want["valid"][8:16, 8:16].any()


@pytest.mark.parametrize("H,W,kind,z_forward,stride", cc.GOLDEN_DEPTH)
def test_novelty_drop_in_against_the_reference(gpu, H, W, kind, z_forward, stride):
    """the mask the reference's own function returned, element for element, shape and dtype included; host and device inputs, the
    environment as a tensor and as a prebuilt index"""
    from fisher_rast.cloud import CloudIndex, novelty_mask_from_pcd_nn
    z = np.load(GOLDEN)
    c = cc.qualifying_depth_case(H, W, kind, z_forward)
    want = z[f"{H}/{W}/{kind}/{z_forward}/{stride}/{c['seed']}/mask"]
    env, inv_K, c2w = torch.from_numpy(c["env"]), torch.from_numpy(c["inv_K"]), torch.from_numpy(c["c2w"])
    for e, pose in ((env, c2w), (env.to(gpu), c2w.to(gpu)), (CloudIndex(env.to(gpu)), c2w)):
        got = novelty_mask_from_pcd_nn(e, c["depth"], inv_K, pose, (H, W), z_forward=z_forward, stride=stride)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert (want.shape == (H, W) and not want.any()) if kind != "object" else want.sum() >= 20


@pytest.mark.parametrize("family,N,M", cc.GOLDEN_POINTS)
def test_metrics_drop_in_against_the_reference(gpu, cloud_harness, family, N, M):
    """acc / comp to relative 1e-6 and ratio exactly, against the reference's own returns; exactly the harness's numbers; and
    reconstruction_metrics equals two drop-in calls with swapped arguments"""
    from fisher_rast.cloud import CloudIndex, accuracy_comp_ratio_from_pcl, reconstruction_metrics
    z = np.load(GOLDEN)
    gt, rec, seed = cc.qualifying_case(family, N, M)
    for th in cc.THRESHOLDS:
        fwd = z[f"{family}/{N}/{M}/{seed}/{th}/forward"]
        a = accuracy_comp_ratio_from_pcl(gt, rec, th)
        b = accuracy_comp_ratio_from_pcl(torch.from_numpy(rec).to(gpu), torch.from_numpy(gt.astype(np.float64)), th)
        assert all(abs(a[k] - fwd[k]) <= 1e-6 * abs(fwd[k]) for k in (0, 1)) and a[2] == fwd[2], (a, fwd)
        m = reconstruction_metrics(CloudIndex(_dev(gt, gpu)), rec, th)
        assert (m["acc"], m["comp"], m["ratio"]) == a and (m["comp"], m["acc"], m["iratio"]) == b and m["fpr"] == 1.0 - b[2]
        assert m == cc.harness_metrics(cloud_harness, gt, rec, th)


def test_an_index_is_reusable(gpu):
    """queried twice, and after another index was built and queried in between: the same bytes"""
    from fisher_rast.cloud import CloudIndex
    t, q, want = _case("clusters", 5000, 1000)
    t2, q2, want2 = _case("uniform", 2049, 257)
    ix, qd = CloudIndex(_dev(t, gpu)), _dev(q, gpu)
    first = ix.search(qd, TH, index=True, flag=True, stats=True)
    other = CloudIndex(_dev(t2, gpu))
    _check(other.search(_dev(q2, gpu), TH, index=True, flag=True, stats=True), want2, "other")
    again = ix.search(qd, TH, index=True, flag=True, stats=True)
    _check(first, want, "first")
    _check(again, want, "again")
    _check(ix.search(_dev(q2, gpu), TH, index=True, flag=True, stats=True), cc.harness_query(cc.build_harness(), t, q2, TH), "smaller workspace need")


def test_empty_and_non_finite_clouds(gpu):
    from fisher_rast.cloud import CloudIndex, decode_stats
    t, q, _ = _case("nonfinite", 1025, 257)
    none = torch.zeros((0, 3), device=gpu)
    n_bad = int((~np.isfinite(q).all(1)).sum())
    assert n_bad > 0
    for targets in (none, torch.full((70, 3), float("nan"), device=gpu), torch.tensor([[0.0, float("inf"), 0.0]], device=gpu)):
        r = CloudIndex(targets).search(_dev(q, gpu), TH, index=True, flag=True, stats=True)
        assert torch.isinf(r["dist"]).all() and (r["dist"] > 0).all() and (r["index"] == -1).all() and not r["flag"].any()
        s = decode_stats(r["stats"].cpu().numpy())
        assert s["sum"] == float("inf") and s["valid"] == len(q) - n_bad and s["flagged"] == 0 and s["skipped"] == n_bad
    r = CloudIndex(_dev(t, gpu)).search(none, TH, index=True, flag=True, stats=True)
    assert r["dist"].shape == (0,) and r["index"].shape == (0,) and r["stats"].cpu().tolist() == [0, 0, 0, 0]
    assert CloudIndex(none).stats(none, TH).cpu().tolist() == [0, 0, 0, 0]


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
    """none in .query, .stats, .query_depth (and the build); exactly one host read in each drop-in and in reconstruction_metrics"""
    from fisher_rast import cloud
    t, q, want = _case("surface", 5000, 1000)
    c = cc.qualifying_depth_case(48, 64, "object", "-Z")
    td, qd, depth, env = _dev(t, gpu), _dev(q, gpu), _dev(c["depth"], gpu), _dev(c["env"], gpu)
    kinv, c2w = cc.depth_kinv(c), torch.from_numpy(c["c2w"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ix = cloud.CloudIndex(td)
        d, i = ix.query(qd, return_index=True)
        s = ix.stats(qd, TH)
        env_ix = cloud.CloudIndex(env)
        mask, ds = env_ix.query_depth(depth, kinv, c2w, stride=2, flip_z=True, dist_th=TH)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    _same(d, want["dist"], "dist")
    _same(i, want["idx"], "idx")
    _same(s, want["stats"], "stats")
    _same(mask, cc.harness_depth(cc.build_harness(), c, 2)["flag"], "mask")
    inv_K = torch.from_numpy(c["inv_K"])
    for name, fn in (("metrics", lambda: cloud.accuracy_comp_ratio_from_pcl(t, q, TH)),
                     ("metrics, device inputs", lambda: cloud.accuracy_comp_ratio_from_pcl(td, qd, TH)),
                     ("reconstruction_metrics", lambda: cloud.reconstruction_metrics(ix, qd, TH)),
                     ("novelty", lambda: cloud.novelty_mask_from_pcd_nn(torch.from_numpy(c["env"]), c["depth"], inv_K, c2w, (48, 64))),
                     ("novelty, prebuilt index", lambda: cloud.novelty_mask_from_pcd_nn(env_ix, c["depth"], inv_K, c2w, (48, 64), stride=2))):
        _, syncs = _syncs(fn)
        print(f"{name}: host synchronisations {len(syncs)}")
        assert len(syncs) == 1, (name, [str(x.message) for x in syncs])


def test_build_and_query_in_stream_order(gpu):
    """build + query (both sources) on a non-default stream, behind a blocker and against a decoy: tests/stream_cases.py's procedure"""
    def make(which):
        t, q = cc.make_case("surface", 2049, 1000, seed=which)
        c = cc.make_depth_case(47, 63, "object", "-Z", seed=which)
        return dict(points=t, queries=q, depth=c["depth"], env=c["env"], kinv=cc.depth_kinv(c), c2w=c["c2w"])

    def call(ctx, b):
        from fisher_rast.cloud import CloudIndex
        r = CloudIndex(b["points"]).search(b["queries"], TH, index=True, flag=True, stats=True)
        mask, dstats, ddist = CloudIndex(b["env"]).query_depth(b["depth"], b["kinv"], b["c2w"], stride=2, flip_z=True, dist_th=TH, want_dist=True)
        return dict(dist=r["dist"], index=r["index"], flag=r["flag"], stats=r["stats"], mask=mask, depth_stats=dstats, depth_dist=ddist)

    case = sc.Case(name="cloud_build_query", make=make, call=call, exact=("dist", "index", "flag", "stats", "mask", "depth_stats", "depth_dist"),
                   same=("kinv",), sync_free=True)
    ref, got = sc.run_case(case, gpu)
    h = cc.build_harness()
    real = make(0)
    _check(got, cc.harness_query(h, real["points"], real["queries"], TH), "stream-ordered run")
    print(f"enqueue {sc.ENQUEUE_MS[case.name]:.3f} ms behind a blocker of {sc.BLOCKER_MS} ms")
