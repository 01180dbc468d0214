"""The running reconstruction metrics without a GPU: the optional fields of fr_cloud_query_cfg (header, ctypes mirror and the layout
a C++ compiler gives the header's struct), the refusals of fr_cloud_query that need no device, the header arithmetic that is new
(csrc/fr_cloud_math.h through tests/harness/fr_recon_harness.cpp), the YAML bookkeeping on hand-computed rows, and the generators of
tests/recon_cases.py: they qualify within the cap on seeds, and the points the product's arithmetic makes are the reference's."""
import ctypes
import os
import re

import numpy as np
import pytest

import cloud_cases as cc
import recon_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def h():
    return rc.build_harness()


def _lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib, _lib.load()


# ---- struct and header ------------------------------------------------------------------------------------------------------------------

def test_new_fields_follow_out_stats_in_header_and_mirror(h):
    _l, _ = _lib()
    names = [n for n, _t in _l.CloudQueryCfg._fields_]
    assert tuple(names) == rc.CFG_FIELDS and names.index("out_stats") + 1 == names.index(rc.NEW_FIELDS[0])
    header = open(os.path.join(ROOT, "include", "fisher_rast.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = plain[plain.index("int32_t source;"):plain.index("} fr_cloud_query_cfg;")]
    declared = re.findall(r"(\w+)\s*[,;]", body)
    assert tuple(declared[declared.index("out_stats") + 1:]) == rc.NEW_FIELDS
    # the layout g++ gives the header's struct is the one ctypes gives the mirror
    size, offsets = rc.cfg_layout(h)
    assert ctypes.sizeof(_l.CloudQueryCfg) == size
    assert {n: getattr(_l.CloudQueryCfg, n).offset for n in names} == offsets


def test_old_keywords_leave_every_new_field_zero():
    _l, _ = _lib()
    A = 1 << 20
    cfg = _l.CloudQueryCfg(source=_l.FR_CLOUD_SOURCE_DEPTH, M=50, H=48, W=64, stride=1, flip_z=1, dist_th=0.05, queries=A, depth=A, kinv=A, c2w=A,
                           out_dist=A, out_idx=A, out_flag=A, out_stats=A)
    for n in rc.NEW_FIELDS:
        assert not getattr(cfg, n), n
    tail = bytes(cfg)[_l.CloudQueryCfg.seed_d2.offset:]
    assert tail == bytes(len(tail))


def test_refusals_need_no_device():
    _l, lib = _lib()
    A, big = 1 << 20, 1 << 40           # addresses that are never dereferenced: every call below is refused on the host

    def query(**kw):
        f = dict(source=_l.FR_CLOUD_SOURCE_POINTS, M=50, H=48, W=64, stride=1, flip_z=0, dist_th=0.05, queries=A, depth=A, kinv=A, c2w=A,
                 out_dist=A, out_idx=None, out_flag=A, out_stats=A)
        f.update(kw)
        cfg = _l.CloudQueryCfg(**f)
        return lib.fr_cloud_query(A, big, 100, ctypes.byref(cfg), A, big, None)

    D = dict(source=_l.FR_CLOUD_SOURCE_DEPTH)
    for bad in (dict(seed_d2=A, out_idx=A), dict(D, seed_d2=A), dict(seed_d2=A + 2), dict(seed_d2=A + 1), dict(mask=A), dict(out_points=A),
                dict(D, out_points=A + 2), dict(D, out_points=A + 1), dict(D, seed_d2=A, mask=A, out_points=A)):
        assert query(**bad) == _l.FR_EINVAL, bad
        assert b"fr_cloud_query" in lib.fr_last_error(), bad


# ---- header arithmetic --------------------------------------------------------------------------------------------------------------------

def _bits(x):
    return np.float32(x).view(np.uint32)


def test_fold_of_a_seed_and_a_candidate(h):
    inf = float("inf")
    rng = np.random.default_rng(1)
    values = [0.0, 1e-45, 1.17549435e-38, 0.5, 1.0, 3.4028235e38, inf] + [float(v) for v in np.abs(rng.normal(size=40)).astype(np.float32) ** 3]
    for x in values:
        assert _bits(h.frc_r_fold(inf, x)) == _bits(x)                                  # +inf and x is x
        assert _bits(h.frc_r_fold(x, inf)) == _bits(x)
        assert _bits(h.frc_r_fold(0.0, x)) == _bits(0.0) == _bits(h.frc_r_fold(x, 0.0))  # 0 and anything is 0
        assert _bits(h.frc_r_fold(x, x)) == _bits(x)                                    # equal values: the bits stay
        assert not h.frc_r_fold_may_improve(x, x)                                       # a tie opens no box
        for y in values:
            got = h.frc_r_fold(x, y)
            assert _bits(got) == _bits(min(np.float32(x), np.float32(y)))
            assert bool(h.frc_r_fold_may_improve(y, x)) == (np.float32(y) < np.float32(x))
    # a candidate one ulp below replaces the seed, one ulp above does not
    x = np.float32(0.3)
    assert _bits(h.frc_r_fold(x, np.nextafter(x, F0))) == _bits(np.nextafter(x, F0)) and _bits(h.frc_r_fold(x, np.nextafter(x, np.float32(1)))) == _bits(x)


F0 = np.float32(0)


def test_fold_of_frames_is_the_search_of_their_union(h):
    """the harness's brute-force fold over the frames of a cut cloud, in both orders, against the brute-force search of the whole"""
    ch = cc.build_harness()
    for family in rc.FOLD_FAMILIES:
        t, q, _ = cc.qualifying_case(family, 1025, 65)
        want = cc.harness_query(ch, t, q, 0.05)["dist"]
        for k in rc.FOLD_K:
            frames = rc.cut(t, k)
            assert sum(len(f) for f in frames) == len(t) and (k < 5 or any(len(f) == 0 for f in frames))
            if family == "nonfinite" and k == 5:
                assert any(len(f) and not np.isfinite(f).all(1).any() for f in frames)
            for order in (frames, frames[::-1]):
                seed = np.full(len(q), np.inf, np.float32)
                for f in order:
                    seed = rc.harness_fold(h, f, q, seed)
                ok = np.isfinite(q).all(1)
                assert np.array_equal(np.sqrt(seed[ok]).view(np.uint32), want[ok].view(np.uint32)), (family, k)
                assert np.isinf(seed[~ok]).all()


def test_masked_sample_predicate(h):
    nan, inf = float("nan"), float("inf")
    for d, valid in ((1.0, True), (1e-30, True), (0.0, False), (-0.0, False), (-1.0, False), (inf, False), (-inf, False), (nan, False)):
        assert bool(h.frc_r_sample_is_query(d, 0, 0)) == valid                          # no mask: the byte is not looked at
        assert bool(h.frc_r_sample_is_query(d, 0, 255)) == valid
        assert not h.frc_r_sample_is_query(d, 1, 0)                                     # masked out: never a query
        for byte in (1, 2, 128, 255):
            assert bool(h.frc_r_sample_is_query(d, 1, byte)) == valid


# ---- the generators -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_gt", [1000, 5000])
def test_object_scene_qualifies_and_its_points_are_the_references(h, n_gt):
    """the cap on seeds is the condition of the GPU test against the float64 statement: the generator meets it here; the points the
    product's arithmetic makes from ONE composed binary32 transform are the reference's two binary64 matmuls to 2e-5 m (coordinates
    below 16 m: 16 * 2^-23 times a few operations), at the same pixels in the same order"""
    s = rc.qualifying_scene(h, n_gt)
    assert s["gt"].shape == (n_gt, 3) and len(s["frames"]) == 5
    total = 0
    for fr in s["frames"]:
        kinv, T = rc.frame_transform(s, fr)
        pts, valid = rc.harness_points(h, fr["depth"], fr["mask"], kinv, T)
        want, want_valid = rc.np_reference_points(s, fr)
        assert np.array_equal(valid.reshape(want_valid.shape), want_valid) and np.isnan(pts[~valid]).all()
        assert np.abs(pts[valid] - want).max() < 2e-5 and np.abs(want).max() < cc.COORD_LIMIT
        masked = fr["mask"] > 0
        assert 50 < valid.sum() < masked.sum() < fr["mask"].size // 2                     # an object mask, with pixels it loses to the depth
        total += int(valid.sum())
    # the metrics move: the object is seen from all round, and the mask's rim of wall pixels keeps the accuracy side away from 0
    d_gt = cc.scipy_nearest(rc.scene_points(h, s), s["gt"])[0]
    d_first = cc.scipy_nearest(rc.scene_points(h, s, 1), s["gt"])[0]
    assert d_gt.mean() < 0.5 * d_first.mean() and (cc.scipy_nearest(s["gt"], rc.scene_points(h, s))[0] > 0.05).any()


# ---- the YAML bookkeeping -------------------------------------------------------------------------------------------------------------------

def _row(step, completeness):
    from fisher_rast.cloud import object_recon_row
    return object_recon_row(step, dict(acc=0.01, comp=0.02, ratio=completeness / 100.0, iratio=0.75, fpr=0.25, n_rec=10), "x.ply")


def test_object_recon_row_has_the_references_keys_and_scaling():
    from fisher_rast import cloud
    row = cloud.object_recon_row(7, dict(acc=0.0125, comp=0.25, ratio=0.5, iratio=0.875, fpr=0.125, n_rec=3), "pointcloud/est.ply")
    assert list(row) == ["step", "acc_distance_m", "comp_distance_m", "completeness_ratio", "fpr", "est_pcl_path"] == list(cloud.RECON_ROW_KEYS)
    assert row == dict(step=7, acc_distance_m=1.25, comp_distance_m=25.0, completeness_ratio=50.0, fpr=12.5, est_pcl_path="pointcloud/est.ply")
    assert all(type(row[k]) is float for k in cloud.RECON_ROW_KEYS[1:5]) and type(row["step"]) is int
    # nothing reconstructed yet: the reference's values for "no cloud file" (all 0), not NaN
    nan = float("nan")
    empty = cloud.object_recon_row(0, dict(acc=nan, comp=float("inf"), ratio=0.0, iratio=nan, fpr=nan, n_rec=0), None)
    assert [empty[k] for k in cloud.RECON_ROW_KEYS[1:5]] == [0.0, 0.0, 0.0, 0.0]


def test_append_recon_row_on_hand_computed_rows():
    from fisher_rast.cloud import append_recon_row, new_recon_data
    data = new_recon_data(0.01, "p", "s")
    assert data == dict(experiment=dict(policy_name="p", scene_id="s"), settings=dict(distance_threshold_m=0.01), steps=[], summary={})
    first = _row(0, 0.0)
    assert append_recon_row(data, first) is data
    assert data["summary"] == dict(auc_completeness_percent_vs_steps_raw=0.0, auc_completeness_normalized_0_1=0.0, last_step=0,
                                   last_completeness_percent=0.0) and first["auc_until_now_normalized"] == 0.0
    # out of order: step 30 before step 10
    last = _row(30, 100.0)
    append_recon_row(data, last)
    assert data["summary"]["auc_completeness_percent_vs_steps_raw"] == 30 * 50.0 and last["auc_until_now_normalized"] == 0.5
    mid = _row(10, 50.0)
    append_recon_row(data, mid)
    assert [r["step"] for r in data["steps"]] == [0, 10, 30] and data["steps"][1] is mid
    assert data["summary"]["auc_completeness_percent_vs_steps_raw"] == 250.0 + 1500.0 == 1750.0
    assert data["summary"]["auc_completeness_normalized_0_1"] == 1750.0 / 3000.0 == mid["auc_until_now_normalized"]
    assert data["summary"]["last_step"] == 30 and data["summary"]["last_completeness_percent"] == 100.0
    # max_steps in the settings: the denominator is max_steps * 100
    capped = new_recon_data(0.01)
    capped["settings"]["max_steps"] = 40
    for r in (_row(0, 0.0), _row(10, 50.0), _row(30, 100.0)):
        append_recon_row(capped, r)
    assert capped["summary"]["auc_completeness_percent_vs_steps_raw"] == 1750.0
    assert capped["summary"]["auc_completeness_normalized_0_1"] == 1750.0 / 4000.0


def test_install_needs_both_methods_and_is_opt_in():
    from fisher_rast import cloud

    class Half:
        def store_filtered_obj_pointcloud(self):
            pass
    with pytest.raises(ValueError, match="evaluate_3d_object_reconstruction"):
        cloud.ReconStreamOps.install(Half)
    import fisher_rast
    assert not hasattr(fisher_rast, "ReconTracker")
    assert np.array_equal(np.array(cloud.ReconStreamOps.HABITAT_TRANSFORM), rc.HABITAT_TRANSFORM)
