"""DBSCAN and the target selection on the CPU: the header (csrc/fr_cluster_math.h, compiled with g++ in
tests/harness/fr_cluster_harness.cpp as a brute-force DBSCAN) against sklearn where it is installed, against the NumPy / cKDTree
restatement of tests/cluster_cases.py and against sklearn's recorded labels (tests/golden/dbscan_cases.npz) -- labels EQUAL, under
the qualification stated there; the cell-adjacency guarantee of the search grid on adversarial pairs; the threshold against
torch.quantile BIT FOR BIT for every n in 1..4096 and a few large n; the winner rule with its quirk and ties; the ABI's rejections,
which need no device; the graft's signature against the reference class where a reference checkout is present."""
import ast
import ctypes
import inspect
import os

import numpy as np
import pytest

import cluster_cases as kc

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dbscan_cases.npz")


@pytest.fixture(scope="module")
def h():
    return kc.build_harness()


def _name(family, N, eps, ms):
    return f"{family}/{N}/{eps:g}/{ms}"


@pytest.mark.parametrize("family,N,eps,ms", kc.GOLDEN)
def test_harness_equals_restatement_and_recorded_sklearn(h, family, N, eps, ms):
    z = np.load(GOLDEN)
    pts, seed = kc.qualifying_case(family, N, eps)
    assert int(z[_name(family, N, eps, ms) + "/seed"]) == seed and kc.qualifies(pts, eps)
    labels, status = kc.harness_dbscan(h, pts, eps, ms)
    assert np.array_equal(labels, kc.restate_dbscan(pts, eps, ms))
    assert np.array_equal(labels, z[_name(family, N, eps, ms) + "/labels"].astype(np.int32))
    assert status[0] == labels.max(initial=-1) + 1 and status[1] == int(np.isfinite(pts).all(1).sum())


@pytest.mark.parametrize("family,N,eps,ms", kc.GOLDEN)
def test_harness_equals_sklearn(h, family, N, eps, ms):
    DBSCAN = pytest.importorskip("sklearn.cluster").DBSCAN
    pts, _ = kc.qualifying_case(family, N, eps)
    ok = np.isfinite(pts).all(1)
    want = np.full(N, -1, np.int64)
    want[ok] = DBSCAN(eps=eps, min_samples=ms).fit(pts[ok]).labels_
    assert np.array_equal(kc.harness_dbscan(h, pts, eps, ms)[0], want)


def test_empty_and_small_clouds(h):
    labels, status = kc.harness_dbscan(h, np.zeros((0, 3), F))
    assert labels.shape == (0,) and not status.any()
    assert kc.harness_dbscan(h, kc.make_case("tiny", 4))[0].tolist() == [-1] * 4                # below min_samples
    assert kc.harness_dbscan(h, kc.make_case("tiny", 5))[0].tolist() == [0] * 5                 # five identical points
    assert kc.harness_dbscan(h, kc.make_case("tiny", 4), min_samples=1)[0].tolist() == [0] * 4  # all within eps of each other
    assert (kc.harness_dbscan(h, kc.make_case("blobs", 65), min_samples=66)[0] == -1).all()      # min_samples > N


def test_border_point_between_two_clusters(h):
    """the clusters must not merge through a point that is not core, and it takes the LOWER label"""
    pts = kc.make_case("bridge", 17)
    labels, status = kc.harness_dbscan(h, pts)
    assert status[0] == 2 and labels[:8].tolist() == [0] * 8 and labels[9:].tolist() == [1] * 8 and labels[8] == 0
    # the other order of the rows: the numbering follows the lowest core index, the border point still takes the lower number
    labels, _ = kc.harness_dbscan(h, pts[::-1].copy())
    assert labels[:8].tolist() == [0] * 8 and labels[9:].tolist() == [1] * 8 and labels[8] == 0


def test_permutation_keeps_the_partition(h):
    pts, _ = kc.qualifying_case("permuted", 1025)
    perm = np.random.default_rng(5).permutation(len(pts))
    a, b = kc.harness_dbscan(h, pts)[0], kc.harness_dbscan(h, pts[perm])[0]
    assert kc.same_partition(a[perm], b) and not np.array_equal(a[perm], b)                      # the same clusters under other numbers
    assert np.array_equal(b, kc.restate_dbscan(pts[perm]))                                      # numbered by the lowest core index of the new order


def test_inclusive_at_an_exactly_representable_distance(h):
    """eps = 0.125: d2 == eps * eps exactly, and the test is <="""
    pts = np.array([[0, 0, 0], [0.125, 0, 0], [0.25, 0, 0], [0.25, 0.1250001, 0]], F)
    assert h.frk_h_inside(kc._p(pts[0]), kc._p(pts[1]), 0.125) == 1 and h.frk_h_dist2(kc._p(pts[0]), kc._p(pts[1])) == F(0.125) * F(0.125)
    assert h.frk_h_inside(kc._p(pts[2]), kc._p(pts[3]), 0.125) == 0
    assert kc.harness_dbscan(h, pts, 0.125, 2)[0].tolist() == [0, 0, 0, -1]


def test_non_finite_points_are_noise_and_nobodys_neighbour(h):
    base = np.zeros((4, 3), F)                                                                  # four identical points: one short of core
    for bad in (np.nan, np.inf, -np.inf):
        pts = np.concatenate([base, np.array([[bad, 0, 0]], F), np.array([[0, bad, 0]], F)])
        labels, status = kc.harness_dbscan(h, pts)
        assert labels.tolist() == [-1] * 6 and status[1] == 4
    assert not h.frk_h_eps_ok(0.0) and not h.frk_h_eps_ok(-0.1) and not h.frk_h_eps_ok(np.nan) and not h.frk_h_eps_ok(1e-20)
    assert not h.frk_h_eps_ok(3e19) and h.frk_h_eps_ok(0.1) and h.frk_h_eps_ok(1.1e-19)


# ---- the grid -----------------------------------------------------------------------------------------------------------------------

def _nudge(x, k):
    """x moved by k units in the last place"""
    x = np.asarray(x, F)
    for _ in range(abs(k)):
        x = np.nextafter(x, F(np.inf if k > 0 else -np.inf))
    return x


@pytest.mark.parametrize("eps", [0.1, 0.125, 0.05, 3.0, 1e-3])
@pytest.mark.parametrize("extent", ["small", "cells", "wide", "huge"])
def test_neighbours_are_at_most_one_cell_apart(h, eps, extent):
    """the guarantee of the header: two points that frk_inside accepts differ by at most one cell on every axis -- pairs straddling
    cell edges, negative coordinates, distances within a few units in the last place of eps, clouds narrower and wider than the grid"""
    rng = np.random.default_rng([int(eps * 1e6), len(extent)])
    side = F(eps) * F(1.125)
    span = dict(small=30 * side, cells=1024 * side, wide=5000 * side, huge=1e7 * side)[extent]
    lo = np.array([-0.37 * span, -span, -1e-3 * span])
    n = 4000
    # p right at (and a few ulps around) a multiple of the expected side above lo; q = p -+ eps (1 + k ulp) along one axis or a diagonal
    step = max(side, span / 1024)
    p = lo + step * rng.integers(1, 1023, (n, 3)) + rng.choice([-1, 0, 1], (n, 3)) * np.spacing(F(span)) * rng.integers(0, 3, (n, 3))
    d = np.zeros((n, 3))
    kind = rng.integers(0, 3, n)
    axis = rng.integers(0, 3, n)
    d[np.arange(n), axis] = 1.0
    diag = kind == 2
    d[diag] = kc._unit(rng, int(diag.sum()))
    sign = rng.choice([-1.0, 1.0], (n, 1))
    scale = float(F(eps)) * (1 + rng.integers(-6, 7, (n, 1)) * 2.0 ** -24) * np.where(kind[:, None] == 1, rng.uniform(0.5, 1.0, (n, 1)), 1.0)
    q = p + sign * d * scale
    corners = np.array([lo, lo + span])                              # fix the frame
    pts = np.ascontiguousarray(np.concatenate([corners, p, q]), F)
    cells, sides = kc.harness_cells(h, pts, eps)
    assert (sides >= side).all() and (cells < 1024).all()
    pc, qc = cells[2:2 + n].astype(np.int64), cells[2 + n:].astype(np.int64)
    inside = np.array([h.frk_h_inside(kc._p(pts[2 + i]), kc._p(pts[2 + n + i]), eps) for i in range(n)], bool)
    assert inside.sum() > n // 10                                     # the property is tested on accepted pairs: there must be some
    assert (np.abs(pc - qc)[inside] <= 1).all(), np.abs(pc - qc)[inside].max()
    if extent in ("small", "cells"):
        assert (sides == side).all()                                  # not coarsened below the cliff
        assert (np.abs(pc - qc)[inside].max() == 1)                   # and pairs do straddle edges


def test_sides_are_per_axis_and_report_the_cliff(h):
    pts = np.zeros((3, 3), F)
    pts[1] = [1e6, 0.5, 0.5]                                          # an outlier in x
    pts[2] = [0.3, 0.2, 0.1]
    _, sides = kc.harness_cells(h, pts, 0.1)
    assert sides[0] == F(1e6) / F(1024) and sides[1] == sides[2] == F(0.1) * F(1.125)
    assert h.frk_h_side(np.inf, -np.inf, 0.1) == F(0.1) * F(1.125)    # no finite point
    assert h.frk_h_cell(3e38, -3e38, np.inf) == 0                     # an extent that overflows: one cell
    assert 0.1 * 1.125 * 1024 > 100                                   # 0.1 m cells cover about 100 m (115.2)


# ---- the threshold ------------------------------------------------------------------------------------------------------------------

def test_threshold_equals_torch_quantile_bit_for_bit(h):
    """every n in 1..4096 and a few large n, q = 0.8 and three more: the fused form of frk_lerp matches torch.quantile on the CPU in
    every bit; a two-rounding a + w (b - a) does not (it differs in the last bit at n = 7, 18, 90, ... for the same data)"""
    import torch
    rng = np.random.default_rng(0)
    naive_misses = 0
    for n in list(range(1, 4097)) + [100003, (1 << 20) + 1, (1 << 24) - 5]:
        x = rng.standard_normal(n).astype(F) if n <= 4096 else rng.random(n, dtype=F)
        for q in ((0.8, 0.5, 0.123, 1.0) if n <= 4096 else (0.8,)):
            want = torch.quantile(torch.from_numpy(x), q).numpy()
            got = kc.harness_quantile(h, x, q)
            assert got.view(np.uint32) == want.view(np.uint32), (n, q, float(got), float(want))
        if n <= 4096:
            s = np.sort(x)
            r = F(0.8) * F(n - 1)
            lo, hi = int(np.floor(r)), int(np.ceil(r))
            naive = F(s[lo] + F(F(r - F(lo)) * F(s[hi] - s[lo])))
            naive_misses += int(naive.view(np.uint32) != torch.quantile(torch.from_numpy(x), 0.8).numpy().view(np.uint32))
    assert naive_misses > 0                                           # the reason the operand order is pinned


def test_threshold_edges(h):
    import torch
    assert kc.harness_quantile(h, np.array([3.5], F)) == F(3.5)
    x = np.array([0.0, -0.0, 1.0, -1.0, 1.0, 1.0], F)                # ties and a signed zero
    for q in (0.0, 0.2, 0.4, 0.8, 1.0):
        assert kc.harness_quantile(h, x, q) == torch.quantile(torch.from_numpy(x), q).numpy()
    out2, w = np.zeros(2, np.uint32), np.zeros(1, F)
    h.frk_h_quantile_rank(0.8, 6, kc._p(out2), kc._p(w))
    assert out2.tolist() == [4, 4] and w[0] == 0                     # an integral rank: the threshold is an element


# ---- the winner and the whole selection ---------------------------------------------------------------------------------------------

def test_winner_rule(h):
    sc = np.array([0.5, 0.9, 0.9, 0.2, 5.0], F)
    assert kc.harness_winner(h, sc, [0, 1, 2, 2, -1]) == 1            # a tie between clusters 1 and 2: the lowest label; noise never wins
    assert kc.harness_winner(h, sc, [2, 1, 0, 0, -1]) == 0
    assert kc.harness_winner(h, sc, [-1] * 5) == -1                   # no cluster: -1, which selects the noise rows
    assert kc.harness_winner(h, np.array([-1.0, -2.0], F), [0, 1]) == -1      # not above the loop's starting score of -1: the quirk
    assert kc.harness_winner(h, np.array([-0.5, -2.0], F), [1, 0]) == 1
    assert kc.harness_winner(h, np.zeros(0, F), np.zeros(0, np.int32)) == -1


def _compare_select(a, want):
    s = a["status"]
    for k in ("band_idx", "above_idx", "labels", "selected_idx"):
        assert np.array_equal(a[k], want[k]), k
    assert np.array_equal(np.asarray(a["threshold"]).view(np.uint32), np.asarray(want["threshold"]).view(np.uint32))
    assert (s["n_band"], s["n_above"], s["n_clusters"], s["max_label"], s["n_selected"], s["argmax"]) == \
           (len(want["band_idx"]), len(want["above_idx"]), want["n_clusters"], want["max_label"], len(want["selected_idx"]), want["argmax"])


def test_selection_equals_the_torch_chain(h):
    means, scores, _ = kc.qualifying_select_case()
    a = kc.harness_select(h, means, scores)
    _compare_select(a, kc.restate_select(means, scores))
    s = a["status"]
    assert s["n_clusters"] >= 2 and 0 < s["n_selected"] < s["n_above"] < s["n_band"] < len(means) and not s["nan"]


def test_selection_edges(h):
    means, scores, _ = kc.qualifying_select_case(kind="equal")
    a = kc.harness_select(h, means, scores)                           # every score equal: nothing is above the threshold
    _compare_select(a, kc.restate_select(means, scores))
    assert a["status"]["n_above"] == 0 and a["status"]["argmax"] == int(a["band_idx"][0]) and a["status"]["max_label"] == -1
    e = kc.harness_select(h, means, scores, lower_y=50.0, upper_y=60.0)       # an empty band
    assert e["status"]["n_band"] == 0 and e["status"]["argmax"] == -1 and np.isnan(e["threshold"])
    scores = scores.copy()
    scores[int(a["band_idx"][3])] = np.nan
    assert kc.harness_select(h, means, scores)["status"]["nan"] == 1
    scores[:] = 0.75
    scores[~((means[:, 1] >= kc.LOWER_Y) & (means[:, 1] <= kc.UPPER_Y))] = np.nan     # NaN outside the band does not raise the flag
    assert kc.harness_select(h, means, scores)["status"]["nan"] == 0
    # no cluster qualifies: max_label stays -1 and the NOISE rows are selected
    sparse = np.stack([np.arange(40) * 1.0, np.zeros(40), np.zeros(40)], 1).astype(F)
    r = kc.harness_select(h, sparse, np.arange(40, dtype=F))
    assert r["status"]["n_clusters"] == 0 and r["status"]["max_label"] == -1 and np.array_equal(r["selected_idx"], r["above_idx"]) and len(r["above_idx"]) == 8


# ---- the ABI, without a device ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from fisher_rast import _lib
    return _lib.load()


def test_workspace_queries(lib):
    from fisher_rast import _lib
    for f in (lib.fr_dbscan_workspace_bytes, lib.fr_target_select_workspace_bytes):
        sizes = [int(f(n)) for n in (0, 1, 255, 256, 257, 5000, 400000, 2000000)]
        assert sizes == sorted(sizes) and sizes[0] > 0 and all(s % 256 == 0 for s in sizes)
        assert f(-1) == 0 and f(_lib.FR_CLUSTER_MAX_POINTS + 1) == 0 and f(_lib.FR_CLUSTER_MAX_POINTS) > 0
    assert lib.fr_target_select_workspace_bytes(5000) > lib.fr_dbscan_workspace_bytes(5000)


def test_abi_rejections(lib):
    from fisher_rast import _lib
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 256
    ok = dict(N=4, points=a, eps=0.1, ms=5, labels=a + 256, status=a + 512, ws=a + 1024, ws_bytes=1 << 30)

    def dbscan(**kw):
        p = {**ok, **kw}
        return lib.fr_dbscan(p["N"], p["points"], p["eps"], p["ms"], p["labels"], p["status"], p["ws"], p["ws_bytes"], None)
    for bad in (dict(N=-1), dict(N=_lib.FR_CLUSTER_MAX_POINTS + 1), dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=1e-25),
                dict(eps=1e30), dict(ms=0), dict(points=None), dict(labels=None), dict(status=None), dict(ws=None), dict(points=a + 2),
                dict(labels=a + 258), dict(ws=a + 1028), dict(ws_bytes=lib.fr_dbscan_workspace_bytes(4) - 1)):
        assert dbscan(**bad) == _lib.FR_EINVAL, bad
        assert b"fr_dbscan" in lib.fr_last_error()

    def select(**kw):
        p = {**dict(P=4, means=a, scores=a + 64, lo=-1.0, hi=1.0, q=0.8, eps=0.1, ms=5, o0=a + 128, o1=a + 192, o2=a + 256, o3=a + 320, thr=a + 384,
                    status=a + 512, ws=a + 1024, ws_bytes=1 << 30), **kw}
        return lib.fr_target_select(p["P"], p["means"], p["scores"], p["lo"], p["hi"], p["q"], p["eps"], p["ms"], p["o0"], p["o1"], p["o2"], p["o3"],
                                    p["thr"], p["status"], p["ws"], p["ws_bytes"], None)
    for bad in (dict(P=-1), dict(q=-0.1), dict(q=1.5), dict(q=float("nan")), dict(eps=0.0), dict(ms=0), dict(means=None), dict(scores=None),
                dict(o0=None), dict(o3=None), dict(thr=None), dict(status=None), dict(ws=None), dict(scores=a + 66), dict(ws=a + 1028),
                dict(ws_bytes=lib.fr_target_select_workspace_bytes(4) - 1)):
        assert select(**bad) == _lib.FR_EINVAL, bad
        assert b"fr_target_select" in lib.fr_last_error()


def test_python_front_end_rejects_bad_arguments_before_any_launch():
    from fisher_rast import cluster
    from fisher_rast._lib import FisherRastError
    with pytest.raises(FisherRastError):
        cluster._check_params(0.0, 5)
    with pytest.raises(FisherRastError):
        cluster._check_params(0.1, 0)
    assert cluster._check_params(np.float32(0.1), np.int64(5)) == (float(np.float32(0.1)), 5)
    assert cluster.TargetSelection._fields[:5] == ("points_index_range", "points_index", "labels", "selected_points_index", "threshold")


# ---- the graft ----------------------------------------------------------------------------------------------------------------------

def test_install_is_opt_in_and_needs_the_fisher_ops():
    from models.SLAM import gaussian as g

    class Bare:
        selection = 0

        def build_frontiers(self):
            return None

        def generate_Gaussian_at_frontier(self):
            return None
    assert not hasattr(g.GaussianSLAM, "global_planning") and not hasattr(g.GaussianSLAM, "select_target_points")
    assert g.TargetSelectOps.install(Bare) is Bare
    with pytest.raises(RuntimeError, match="FisherOps and PointScoreOps"):
        Bare().global_planning(None, np.eye(4))
    src = inspect.getsource(g.FisherOps.install)
    assert "TargetSelectOps" not in src and "global_planning" not in src            # FisherOps.install does not install it


def _reference_root():
    for cand in (os.environ.get("FISHER_REFERENCE"), os.path.join(os.path.dirname(ROOT), "reference")):
        if cand and os.path.exists(os.path.join(cand, "models", "SLAM", "gaussian.py")):
            return cand
    return None


@pytest.mark.parametrize("ref_file,ref_cls", [("models/SLAM/gaussian.py", "GaussianSLAM"), ("models/SLAM/gaussian_object.py", "GaussianObjectSLAM")])
def test_global_planning_signature_against_the_reference(ref_file, ref_cls):
    """same positional parameters in the same order (the reference source is PARSED, nothing of it is imported or executed)"""
    root = _reference_root()
    if root is None:
        pytest.skip("no reference checkout beside the repository (FISHER_REFERENCE)")
    from models.SLAM.gaussian import TargetSelectOps
    tree = ast.parse(open(os.path.join(root, ref_file)).read())
    cls = next(n for n in ast.walk(tree) if isinstance(n, ast.ClassDef) and n.name == ref_cls)
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "global_planning")
    ref = [a.arg for a in fn.args.args]
    ours = list(inspect.signature(TargetSelectOps.global_planning).parameters)
    assert ours == ref == ["self", "follower", "agent_pose"]
    assert not fn.args.defaults and not fn.args.kwonlyargs
