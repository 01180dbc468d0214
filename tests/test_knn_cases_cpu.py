"""The cases of tests/knn_cases.py qualified without a GPU: conditions on the inputs, not on the code.  What is used: the
brute-force oracle (orc_knn_dist2), the NumPy restatement of k_knn_morton and SciPy's cKDTree in float64.

Measured with these generators (seed 0): `seam` has a nearest neighbour at least 1024 ranks away for 0.35 / 0.65 / 0.83 of its
points at P = 4097 / 8193 / 16385 and one at least 64 ranks away for 0.84 / 0.84 / 0.85; a uniform cloud of 8193 points gives 0.08
and 0.34.  `stretch` has code 0 for 0.9995 of its points at P = 2049 and 0.9998 at P = 5000."""
import numpy as np
import pytest

import knn_cases as kc


@pytest.mark.parametrize("P", kc.SEAM_SIZES)
def test_seam_neighbours_lie_far_along_the_curve(P):
    box, sub = kc.far_neighbour_fractions(kc.make_cloud("seam", P))
    print(f"seam P={P}: a neighbour >= 1024 ranks away {box:.3f}, >= 64 ranks away {sub:.3f}")
    assert box >= kc.SEAM_FAR_BOX and sub >= kc.SEAM_FAR_SUB


def test_a_uniform_cloud_would_not_do():
    box, sub = kc.far_neighbour_fractions(kc.make_cloud("uniform", 8193))
    print(f"uniform P=8193: {box:.3f}, {sub:.3f}")
    assert box < kc.SEAM_FAR_BOX / 2 and sub < kc.SEAM_FAR_SUB / 2


@pytest.mark.parametrize("P", sorted(set(kc.KNN_FAMILY_SIZES["stretch"] + kc.ORDER_FAMILY_SIZES["stretch"])))
def test_stretch_quantises_to_code_zero(P):
    m = kc.make_cloud("stretch", P)
    f = kc.code0_fraction(m)
    print(f"stretch P={P}: code 0 for {f:.4f}")
    assert f >= kc.STRETCH_CODE0
    # the order of those points is the index order
    zero = np.flatnonzero(kc.morton_np(m) == 0)
    assert np.array_equal(kc.z_order(m)[:len(zero)], zero)


@pytest.mark.parametrize("family", ["plane", "line", "point"])
def test_degenerate_axes(family):
    for P in kc.KNN_FAMILY_SIZES[family]:
        m = kc.make_cloud(family, P)
        held = (m.max(0) == m.min(0)).sum() if P > 1 else 3
        assert held == dict(plane=1, line=2, point=3)[family]
    if family == "point":
        assert not kc.morton_np(m).any()


@pytest.mark.parametrize("P", kc.KNN_FAMILY_SIZES["lattice"])
def test_lattice_answer_is_closed_form(oracle, P):
    want = oracle.knn_dist2(kc.make_cloud("lattice", P))
    assert np.array_equal(kc.bits(want), kc.bits(np.full(P, kc.LATTICE_ANSWER)))


@pytest.mark.parametrize("P", kc.KNN_FAMILY_SIZES["point"])
def test_point_answer_is_zero(oracle, P):
    assert P >= 4 and not kc.bits(oracle.knn_dist2(kc.make_cloud("point", P))).any()


@pytest.mark.parametrize("P", kc.KNN_FAMILY_SIZES["dup_groups"])
def test_dup_groups_answers(oracle, P):
    m = kc.make_cloud("dup_groups", P)
    want = oracle.knn_dist2(m)
    groups = kc.dup_group_rows(P)
    assert sorted({len(g) for g in groups}) == [2, 3, 4, 5]
    for g in groups:
        assert (m[g] == m[g[0]]).all() and len(np.unique(kc.bits(want[g]))) == 1
        assert (want[g] > 0).all() if len(g) <= 3 else not kc.bits(want[g]).any(), (len(g), want[g])
    rest = np.setdiff1d(np.arange(P), np.concatenate(groups))
    assert (want[rest] > 0).all()


@pytest.mark.parametrize("P", kc.KNN_FAMILY_SIZES["nonfinite"])
def test_nonfinite_rows_are_inert(oracle, P):
    m = kc.make_cloud("nonfinite", P)
    bad = ~np.isfinite(m).all(1)
    assert 0.03 * P < bad.sum() < 0.08 * P and np.isnan(m).any() and (m == np.inf).any() and (m == -np.inf).any()
    want = oracle.knn_dist2(m)
    assert (kc.bits(want[bad]) == 0x7F800000).all()
    assert np.array_equal(kc.bits(want[~bad]), kc.bits(oracle.knn_dist2(m[~bad])))
    # the NaN-only variant keeps finite bounds, so its codes are not all equal
    nan_only = kc.make_cloud("nonfinite", P, kinds=(np.nan,))
    code = kc.morton_np(nan_only)
    assert np.isnan(nan_only).any(1).sum() == bad.sum() and len(np.unique(code)) > P // 2
    # with an infinity on every axis every extent is infinite and every code is 0
    assert not kc.morton_np(m).any()


@pytest.mark.parametrize("P", kc.KNN_FAMILY_SIZES["overflow"])
def test_overflow_leaves_best_at_flt_max(oracle, P):
    """every squared distance is inf, so `best` stays at FLT_MAX three times and their sum is inf"""
    assert (kc.bits(oracle.knn_dist2(kc.make_cloud("overflow", P))) == 0x7F800000).all()


def test_offset_frame_is_far_from_the_origin():
    m = kc.make_cloud("offset", 5000)
    assert np.abs(m.mean(0) - np.array([1000, -500, 2000])).max() < 0.01 and (m.max(0) - m.min(0)).max() < 0.2


def test_scaling_law_of_the_oracle(oracle):
    m = np.random.default_rng(7).normal(size=(kc.SCALING_P, 3)).astype(np.float32)
    assert kc.scaling_mismatches(oracle.knn_dist2, m) == [0, 0]
    # the cloud of the GPU's metamorphic checks obeys it too: no row's arithmetic leaves the normal range
    m = kc.metamorphic_cloud()
    assert kc.scaling_mismatches(oracle.knn_dist2, m) == [0, 0]
    assert (oracle.knn_dist2(m) == 0).sum() >= 50


@pytest.mark.parametrize("pattern", kc.PATTERNS)
def test_patterns_have_the_wanted_codes(pattern):
    for P in kc.PATTERN_SIZES:
        q, code = kc.pattern_codes(pattern, P)
        m = kc.pattern_points(pattern, P)
        assert m.shape == (P, 3) and np.array_equal(kc.morton_np(m), code)
        mid = code[1:-1]
        if pattern == "equal":
            assert len(np.unique(mid)) == 1 and np.array_equal(kc.z_order(m), np.arange(P))
        elif pattern == "descending":
            assert (code[1:] < code[:-1]).all() and np.array_equal(kc.z_order(m), np.arange(P)[::-1])
        else:
            zero, one = kc.encode([kc.ZERO_CELL])[0], kc.encode([kc.ONE_CELL])[0]
            assert 0 < zero < one < code[0] and set(np.unique(mid)) == {zero, one} and code[-1] == 0        # corners swapped
            assert kc.z_order(m)[0] == P - 1 and kc.z_order(m)[-1] == 0
            ones = int((mid == one).sum())
            want = dict([("ones-then-zeros", (P - 2) // 2), ("alternating", (P - 1) // 2), ("one-in-front", 1), ("zero-at-the-end", P - 3)]).get(pattern)
            assert ones == want if want is not None else 0 < ones < P - 2


def test_restatement_on_finite_clouds_is_the_min_max_form():
    """the fmin / fmax bounds and the NaN rule change nothing for finite points"""
    m = kc.make_cloud("uniform", 5000)
    lo, hi = m.min(0), m.max(0)
    q = (np.clip((m - lo) / (hi - lo), 0, 1).astype(np.float32) * np.float32(1023.0)).astype(np.uint32)
    assert np.array_equal(kc.morton_np(m), kc.encode(q))
    from test_gpu_spatial_order import _morton_np
    assert _morton_np is kc.morton_np
