"""The nearest-point search on the CPU: the arithmetic (csrc/fr_cloud_math.h, compiled with g++ in tests/harness/fr_cloud_harness.cpp,
a brute-force search with lowest-index ties) against the SciPy float64 statement of tests/cloud_cases.py on every family and size;
the product's host arithmetic over the harness against the outputs of the reference's own functions
(tests/golden/reference_cloud.npz) on the cases that qualify; the box bound as a property; the ABI's rejections, which need no
device; the drop-ins' signatures and the install.

Distances: relative 1e-6, zeros exact.  Derived bound for binary32 against binary64 on float32 inputs: a subtraction, three squares,
two additions and a square root are at most 8 roundings of 2^-24 in the squared distance's worth, 8 * 2^-24 = 4.8e-7."""
import ctypes
import inspect
import json
import os
import types

import numpy as np
import pytest

import cloud_cases as cc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_cloud.npz")
REL = 1e-6


@pytest.fixture(scope="module")
def cloud_harness():
    return cc.build_harness()


def _close(got, want, rel=REL):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    return bool((same | (np.abs(got - want) <= rel * np.abs(want))).all())


def _check_against_scipy(h, t, q, family):
    d64, i64 = cc.scipy_nearest(t, q)
    assert cc.qualifies_points(t, q, d64=d64)
    worst = 0.0
    for th in cc.THRESHOLDS:
        r = cc.harness_query(h, t, q, th)
        ok = np.isfinite(q).all(1)
        has_target = np.isfinite(t).all(1).any()
        # a query that is not finite: +inf / -1 / no flag, counted as skipped
        assert np.isinf(r["dist"][~ok]).all() and (r["idx"][~ok] == -1).all() and not r["flag"][~ok].any()
        if not has_target:
            assert np.isinf(r["dist"]).all() and (r["idx"] == -1).all()
            continue
        d = r["dist"][ok].astype(np.float64)
        assert _close(d, d64[ok]), (family, np.abs(d - d64[ok]).max())
        assert ((d64[ok] == 0) == (d == 0)).all()                                       # zeros exact
        nz = d64[ok] > 0
        worst = max(worst, float((np.abs(d - d64[ok])[nz] / d64[ok][nz]).max(initial=0.0)))
        # the index attains the distance, is a finite target, and no lower index attains it
        idx = r["idx"][ok]
        assert (idx >= 0).all() and np.isfinite(t[idx]).all()
        dd = q[ok].astype(np.float32) - t[idx]
        d2 = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
        assert np.array_equal(np.sqrt(d2).view(np.uint32), r["dist"][ok].view(np.uint32))
        # flags and statistics
        s = cc.decode(r["stats"])
        assert s["valid"] == int(ok.sum()) and s["skipped"] == int((~ok).sum())
        assert s["flagged"] == int((d64[ok] < th).sum()) == int(r["flag"].sum())
        assert np.array_equal(r["flag"][ok].astype(bool), d64[ok] < th)
        assert _close(s["sum"], d64[ok].sum())
    return worst


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_harness_against_scipy_float64(cloud_harness, family):
    """distances to relative 1e-6 with zeros exact, flag counts and statistics equal under the qualification, at every size"""
    worst = 0.0
    sizes = [(N, M) for N in cc.N_SIZES for M in cc.M_SIZES] + [(cc.N_LARGE, 1000)]
    for N, M in sizes:
        t, q, _ = cc.qualifying_case(family, N, M)
        worst = max(worst, _check_against_scipy(cloud_harness, t, q, family))
    print(f"{family}: worst relative distance error against float64 {worst:.2e}")
    assert worst <= REL


def test_lowest_index_wins_a_tie(cloud_harness):
    t = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0], [np.nan, 0, 0]], np.float32)
    q = np.array([[0, 0, 0], [1, 0, 0], [np.inf, 0, 0]], np.float32)
    r = cc.harness_query(cloud_harness, t, q, 0.5)
    assert r["idx"].tolist() == [0, 0, -1] and r["dist"].tolist() == [1.0, 0.0, np.inf] and r["flag"].tolist() == [0, 1, 0]
    assert cc.decode(r["stats"]) == dict(sum=1.0, valid=2, flagged=1, skipped=1)
    # no target at all, no finite target, no query
    for tt in (np.zeros((0, 3), np.float32), t[4:]):
        r = cc.harness_query(cloud_harness, tt, q, 0.5)
        assert np.isinf(r["dist"]).all() and (r["idx"] == -1).all() and not r["flag"].any()
    assert cc.decode(cc.harness_query(cloud_harness, t, np.zeros((0, 3), np.float32), 0.5)["stats"]) == dict(sum=0.0, valid=0, flagged=0, skipped=0)


@pytest.mark.parametrize("family,N,M", cc.GOLDEN_POINTS)
def test_metrics_against_scipy_and_the_reference(cloud_harness, family, N, M):
    """acc / comp to relative 1e-6, ratio exactly equal: against the float64 statement and against what the reference's own function
    returned, for both orders of the arguments"""
    z = np.load(GOLDEN)
    gt, rec, seed = cc.qualifying_case(family, N, M)
    name = f"{family}/{N}/{M}/{seed}"
    assert name in [str(k) for k in z["points_cases"]] and cc.qualifies_points(rec, gt)
    for th in cc.THRESHOLDS:
        m = cc.harness_metrics(cloud_harness, gt, rec, th)
        fwd, swp = z[f"{name}/{th}/forward"], z[f"{name}/{th}/swapped"]
        for want in (cc.scipy_metrics(gt, rec, th), tuple(fwd)):
            assert _close(m["acc"], want[0]) and _close(m["comp"], want[1]) and m["ratio"] == want[2], (m, want)
        assert _close(m["comp"], swp[0]) and _close(m["acc"], swp[1]) and m["iratio"] == swp[2] and m["fpr"] == 1.0 - swp[2]
        assert cc.harness_metrics(cloud_harness, rec, gt, th)["ratio"] == m["iratio"]


def _depth_golden():
    return [(H, W, kind, zf, stride) for H, W, kind, zf, stride in cc.GOLDEN_DEPTH]


@pytest.mark.parametrize("H,W,kind,z_forward,stride", _depth_golden())
def test_novelty_mask_against_the_reference(cloud_harness, H, W, kind, z_forward, stride):
    """the mask equal element for element, shape and dtype included -- the < 20 novel and none-valid returns have the FULL shape"""
    z = np.load(GOLDEN)
    c = cc.qualifying_depth_case(H, W, kind, z_forward)
    name = f"{H}/{W}/{kind}/{z_forward}/{stride}/{c['seed']}"
    assert name in [str(k) for k in z["depth_cases"]]
    want = z[name + "/mask"]
    got = cc.harness_novelty_mask(cloud_harness, c, stride)
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)
    assert got.max(initial=0) <= 1
    if kind == "object":
        assert got.shape == ((H + stride - 1) // stride, (W + stride - 1) // stride) and got.sum() >= 20
    else:
        assert got.shape == (H, W) and not got.any()
    novel = cc.decode(cc.harness_depth(cloud_harness, c, stride)["stats"])["flagged"]
    assert (1 <= novel <= 19) if kind == "few" else (novel == 0 if kind == "none-valid" else novel >= 20)


@pytest.mark.parametrize("H,W", cc.DEPTH_SHAPES)
@pytest.mark.parametrize("z_forward", ["-Z", "Z"])
def test_depth_mode_against_the_float64_statement(cloud_harness, H, W, z_forward):
    for kind in cc.DEPTH_KINDS:
        c = cc.qualifying_depth_case(H, W, kind, z_forward)
        for stride in (1, 2, 3):
            r = cc.harness_depth(cloud_harness, c, stride)
            pw, valid = cc.np_depth_points(c, stride)
            assert np.array_equal(r["valid"].astype(bool), valid)
            assert np.abs(r["points"][valid] - pw[valid]).max(initial=0.0) < 2e-5          # 16 m * 2^-23 * a few operations
            s = cc.decode(r["stats"])
            assert s["valid"] == int(valid.sum()) and s["skipped"] == int((~valid).sum())
            assert not r["flag"][~valid].any() and np.isinf(r["dist"][~valid]).all() and (r["idx"][~valid] == -1).all()
            if valid.any():
                d64 = cc.scipy_nearest(c["env"], pw[valid])[0]
                assert np.array_equal(r["flag"][valid].astype(bool), d64 > 0.05) and s["flagged"] == int((d64 > 0.05).sum())
            assert np.array_equal(cc.harness_novelty_mask(cloud_harness, c, stride), cc.scipy_novelty_mask(c, stride))


def test_box_bound_never_exceeds_the_distance(cloud_harness):
    """the header's box bound against the header's distance for points inside random and degenerate boxes: compared as floats"""
    h = cloud_harness
    rng = np.random.default_rng(5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n_outside = 0
    for trial in range(4000):
        scale = 10.0 ** rng.integers(-3, 2)
        lo = (rng.uniform(-1, 1, 3) * scale).astype(np.float32)
        ext = (rng.uniform(0, 1, 3) * scale * 10.0 ** rng.integers(-4, 1)).astype(np.float32)
        ext[rng.uniform(size=3) < 0.2] = 0.0                                                # a plane, a line, a point
        hi = (lo + ext).astype(np.float32)
        q = (lo + rng.normal(0, 1, 3) * scale * 10.0 ** rng.integers(-4, 1)).astype(np.float32)
        if trial % 7 == 0:
            q[rng.integers(0, 3)] = (lo if trial % 2 else hi)[0]                             # on a face's coordinate
        bound = h.frc_h_box_dist2(p(q), p(lo), p(hi))
        n_outside += bound > 0
        u = rng.uniform(0, 1, (24, 3))
        u[:8] = rng.integers(0, 2, (8, 3))                                                  # the corners
        ts = np.clip((lo + u * (hi - lo)).astype(np.float32), lo, hi)
        for t in ts:
            t = np.ascontiguousarray(t)
            assert bound <= h.frc_h_dist2(p(q), p(t)), (q, lo, hi, t)
    assert n_outside > 1000
    # the box no point was put into: its bound is +inf
    inf = np.full(3, np.inf, np.float32)
    assert h.frc_h_box_dist2(p(np.zeros(3, np.float32)), p(inf), p(-inf)) == np.inf


def test_morton_clamps_outside_queries(cloud_harness):
    h = cloud_harness
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lo, hi = np.array([-1, -1, -1], np.float32), np.array([1, 1, 1], np.float32)
    code = lambda *q: h.frc_h_morton(p(np.array(q, np.float32)), p(lo), p(hi))
    assert code(-50, -50, -50) == code(-1, -1, -1) == 0 and code(50, 50, 50) == code(1, 1, 1) == (1 << 30) - 1
    assert code(0, 0, 0) < code(0.5, 0.5, 0.5) < (1 << 30)
    assert h.frc_h_morton(p(np.zeros(3, np.float32)), p(lo), p(lo)) == 0                      # zero extent


# ---- the ABI, without a device --------------------------------------------------------------------------------------------------------

def _lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib, _lib.load()


def test_sizes_are_host_only_and_monotone():
    _l, lib = _lib()
    assert lib.fr_version() == 100
    for f in (lib.fr_cloud_index_bytes, lib.fr_cloud_index_workspace_bytes, lib.fr_cloud_query_workspace_bytes):
        sizes = [int(f(n)) for n in (0, 1, 63, 64, 65, 1024, 1025, 5000, 500000, 2000000, _l.FR_CLOUD_MAX_POINTS)]
        assert all(b >= a > 0 for a, b in zip(sizes, sizes[1:])), sizes
        assert f(-1) == 0 and f(_l.FR_CLOUD_MAX_POINTS + 1) == 0
    assert lib.fr_cloud_index_bytes(1000) >= 1000 * 20 and lib.fr_cloud_query_workspace_bytes(1000) >= 1000 * 12


def test_abi_rejections_need_no_device():
    _l, lib = _lib()
    A, big = 1 << 20, 1 << 40           # addresses that are never dereferenced: every call below is refused on the host

    def build(N=100, points=A, index=A, nix=big, ws=A, nws=big):
        return lib.fr_cloud_index_build(N, points, index, nix, ws, nws, None)

    for bad in (dict(N=-1), dict(N=_l.FR_CLOUD_MAX_POINTS + 1), dict(points=None), dict(index=None), dict(ws=None), dict(points=A + 2),
                dict(index=A + 4), dict(ws=A + 4), dict(nix=int(lib.fr_cloud_index_bytes(100)) - 1), dict(nix=0),
                dict(nws=int(lib.fr_cloud_index_workspace_bytes(100)) - 1)):
        assert build(**bad) == _l.FR_EINVAL, bad
        assert b"fr_cloud_index_build" in lib.fr_last_error()

    def query(index=A, nix=big, N=100, ws=A, nws=big, no_cfg=False, **kw):
        f = dict(source=_l.FR_CLOUD_SOURCE_POINTS, M=50, H=48, W=64, stride=1, flip_z=0, dist_th=0.05, queries=A, depth=A, kinv=A, c2w=A,
                 out_dist=A, out_idx=A, out_flag=A, out_stats=A)
        f.update(kw)
        cfg = _l.CloudQueryCfg(**f)
        return lib.fr_cloud_query(index, nix, N, None if no_cfg else ctypes.byref(cfg), ws, nws, None)

    D = dict(source=_l.FR_CLOUD_SOURCE_DEPTH)
    for bad in (dict(index=None), dict(no_cfg=True), dict(ws=None), dict(N=-1), dict(N=_l.FR_CLOUD_MAX_POINTS + 1), dict(source=2), dict(source=-1),
                dict(M=-1), dict(M=_l.FR_CLOUD_MAX_POINTS + 1), dict(queries=None), dict(queries=A + 1), dict(index=A + 4), dict(ws=A + 4),
                dict(out_dist=A + 2), dict(out_idx=A + 2), dict(out_stats=A + 4), dict(nix=int(lib.fr_cloud_index_bytes(100)) - 1),
                dict(nws=int(lib.fr_cloud_query_workspace_bytes(50)) - 1), dict(nws=0),
                dict(D, H=0), dict(D, W=0), dict(D, H=-4), dict(D, stride=0), dict(D, stride=-1), dict(D, depth=None), dict(D, kinv=None),
                dict(D, c2w=None), dict(D, depth=A + 2), dict(D, kinv=A + 1), dict(D, c2w=A + 3), dict(D, H=1 << 14, W=1 << 14),
                dict(D, nws=int(lib.fr_cloud_query_workspace_bytes(48 * 64)) - 1)):
        assert query(**bad) == _l.FR_EINVAL, bad
        assert b"fr_cloud_query" in lib.fr_last_error()


def test_sources_exports_and_header():
    from fisher_rast import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert os.path.join(_lib._CSRC, "fr_cloud.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_cloud_math.h") in _lib.SOURCES
    header = open(os.path.join(root, "include", "fisher_rast.h")).read()
    for name in ("fr_cloud_index_bytes", "fr_cloud_index_workspace_bytes", "fr_cloud_query_workspace_bytes", "fr_cloud_index_build", "fr_cloud_query"):
        assert name in _lib.EXPORTS and name + "(" in header
    # the mirrored constants and the struct
    for const in ("FR_CLOUD_STATS_WORDS", "FR_CLOUD_SOURCE_POINTS", "FR_CLOUD_SOURCE_DEPTH"):
        assert f"#define {const} {getattr(_lib, const)}" in header
    assert "#define FR_CLOUD_MAX_POINTS (1 << 27)" in header and _lib.FR_CLOUD_MAX_POINTS == 1 << 27
    import re
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = plain[plain.index("int32_t source;"):plain.index("} fr_cloud_query_cfg;")]
    declared = re.findall(r"(\w+)\s*[,;]", body)
    assert declared == [n for n, _ in _lib.CloudQueryCfg._fields_], declared
    # the sort is shared, not copied
    src = open(os.path.join(root, "fisher-nerf-customized_amd", "csrc", "fr_cloud.hip")).read()
    assert "fr_sort_keys64(" in src and "bitonic" not in src.replace("the bitonic", "")
    assert "atomicAdd(float" not in src and "getenv" not in src and "hipMalloc" not in src and "hipMemcpy(" not in src


# ---- the drop-ins' surface ------------------------------------------------------------------------------------------------------------

def test_signatures_match_the_reference():
    from fisher_rast import cloud
    z = np.load(GOLDEN)
    for name in ("accuracy_comp_ratio_from_pcl", "novelty_mask_from_pcd_nn"):
        want = json.loads(str(z["sig/" + name]))
        got = [[p.name, None if p.default is inspect.Parameter.empty else p.default, p.default is not inspect.Parameter.empty]
               for p in inspect.signature(getattr(cloud, name)).parameters.values()]
        assert got == want, (name, got, want)


def test_install_replaces_the_names_a_module_has():
    from fisher_rast import cloud
    keep = object()
    both = types.ModuleType("fake_tester")
    both.accuracy_comp_ratio_from_pcl = both.novelty_mask_from_pcd_nn = both.other = keep
    assert cloud.CloudEvalOps.install(both) is both
    assert both.accuracy_comp_ratio_from_pcl is cloud.accuracy_comp_ratio_from_pcl and both.novelty_mask_from_pcd_nn is cloud.novelty_mask_from_pcd_nn
    assert both.other is keep
    one = types.ModuleType("fake_eval")
    one.accuracy_comp_ratio_from_pcl = keep
    cloud.CloudEvalOps.install(one)
    assert one.accuracy_comp_ratio_from_pcl is cloud.accuracy_comp_ratio_from_pcl and not hasattr(one, "novelty_mask_from_pcd_nn")
    with pytest.raises(ValueError, match="accuracy_comp_ratio_from_pcl"):
        cloud.CloudEvalOps.install(types.ModuleType("fake_empty"))
    # opt-in: nothing of the package is touched on import
    import fisher_rast
    assert not hasattr(fisher_rast, "accuracy_comp_ratio_from_pcl")


def test_host_arithmetic_of_the_metrics_and_the_mask():
    from fisher_rast import cloud
    a, b = dict(sum=3.0, valid=4, flagged=1, skipped=0), dict(sum=1.0, valid=2, flagged=2, skipped=5)
    assert cloud.metrics_from_stats(a, b) == dict(acc=0.75, comp=0.5, ratio=1.0, iratio=0.25, fpr=0.75)
    empty = cloud.metrics_from_stats(dict(sum=0.0, valid=0, flagged=0, skipped=0), b)
    assert np.isnan(empty["acc"]) and np.isnan(empty["iratio"]) and empty["comp"] == 0.5
    words = np.array([np.float64(2.5).view(np.int64), 7, 3, 1], np.int64)
    assert cloud.decode_stats(words) == dict(sum=2.5, valid=7, flagged=3, skipped=1)
    sub = np.ones((3, 4), np.uint8)
    assert cloud.novelty_mask_from_host(sub, dict(valid=12, flagged=20), 6, 8) is sub
    for s in (dict(valid=12, flagged=19), dict(valid=0, flagged=0)):
        m = cloud.novelty_mask_from_host(sub, s, 6, 8)
        assert m.shape == (6, 8) and m.dtype == np.uint8 and not m.any()
