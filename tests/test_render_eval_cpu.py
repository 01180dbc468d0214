"""The render-quality evaluation without a device: the arithmetic of csrc/fr_eval_math.h through the g++ harness
(tests/harness/fr_eval_harness.cpp) against the reference's own binary32 / binary64 runs (tests/golden/reference_eval.npz), the byte
targets, the summary's keep rule, and the host side of the ABI."""
import ctypes
import os

import numpy as np
import pytest

import eval_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eval_harness():
    return ec.build_harness()


@pytest.fixture(scope="module")
def fixture():
    return ec.load_fixture()


@pytest.fixture(scope="module")
def lib():
    from fisher_rast import _lib
    return _lib.load()


def test_fixture_covers_every_case(fixture):
    want = {ec.key(*c) for c in ec.all_cases()}
    assert set(fixture) == want
    for shape, rot, kind, clamp in ec.all_cases():
        assert fixture[ec.key(shape, rot, kind, clamp)].shape == (shape[0], 2, len(ec.REF_NAMES))
    fams = {f for shape, rot, kind, clamp in ec.all_cases() for f in ec.make_batch(shape, rot, "none")["families"]}
    assert fams == set(ec.FAMILIES)


@pytest.mark.parametrize("family", ec.FAMILIES)
@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_harness_against_the_reference_by_the_rule(eval_harness, fixture, shape, family):
    """Every value of every view of `family` within 2 D_ref + 64 2^-24 |value| of the reference's binary64 run, D_ref the deviation of
    the reference's own binary32 run (loss_cases.tolerance's rule); prints the measured need (deviation / bound).

    Measured, worst over the shapes, masks, clamp settings and both depth forms:
        family        psnr    ssim    depth_l1  depth_rmse
        noise         0.0099  0.019   0.012     0.011
        smooth        0.011   0.036   0.014     0.015
        step          0.012   0.055   0.011     0.013
        identical     0       0       0.013     0.015
        near          0.012   0.010   0.011     0.013
        out_of_range  0.014   0.024   0.013     0.012
        black_gt      0.012   0.029   0.014     0.012
    With fr_loss_math.h's moments about 0.5 alone the SSIM of black_gt needed 15.2 / 17.4 / 19.1 / 17.7 times the bound at the four
    shapes (their absolute error of ~3e-8 against c1 = 1e-4, where the reference's raw moments are exactly 0); a window whose mean is
    below 2^-5 in either image takes the raw moments instead (fr_eval_math.h: fre_window_is_dark)."""
    worst = dict(psnr=0.0, ssim=0.0, depth_l1=0.0, depth_rmse=0.0)
    names = {ec.PSNR: "psnr", ec.SSIM: "ssim", ec.DEPTH_L1: "depth_l1", ec.DEPTH_RMSE: "depth_rmse"}
    failures, checked = [], 0
    for s, rot, kind, clamp in ec.all_cases():
        if s != shape:
            continue
        b = ec.make_batch(s, rot, kind)
        if family not in b["families"]:
            continue
        ref = fixture[ec.key(s, rot, kind, clamp)]
        for valid_only in (False, True):
            rows, _ = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"], b["depth"], b["gt_depth"], b["mask"], clamp, valid_only)
            for v in range(s[0]):
                if b["families"][v] != family:
                    continue
                checked += 1
                for idx, r32, r64 in ec.row_refs(ref[v], valid_only):
                    n = ec.need(rows[v, idx], r32, r64)
                    worst[names[idx]] = max(worst[names[idx]], n)
                    if not n <= 1.0:
                        failures.append((ec.key(s, rot, kind, clamp), v, names[idx], valid_only, float(rows[v, idx]), float(r32), float(r64), n))
                want_cnt = float((b["gt_depth"][v] > 0).sum()) if valid_only else float(s[1] * s[2])
                assert rows[v, ec.DEPTH_COUNT] == want_cnt
    print(f"need {shape} {family}: " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    assert checked > 0
    assert not failures, failures[:4]


def test_special_values_sit_where_the_reference_has_them(eval_harness, fixture):
    """identical and empty-mask views: PSNR +inf; identical: SSIM exactly 1; valid-only without a valid depth: NaN"""
    seen = dict(identical=0, empty=0, novalid=0)
    for s, rot, kind, clamp in ec.all_cases():
        b = ec.make_batch(s, rot, kind)
        ref = fixture[ec.key(s, rot, kind, clamp)]
        rows, _ = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"], b["depth"], b["gt_depth"], b["mask"], clamp, True)
        for v, fam in enumerate(b["families"]):
            if fam == "identical":
                assert rows[v, ec.PSNR] == np.inf and rows[v, ec.SSIM] == 1.0 and ref[v, 1, 0] == np.inf
                assert np.all(rows[v, ec.MSE_R:ec.MSE_B + 1] == 0.0)
                seen["identical"] += 1
            if kind == "empty":
                assert rows[v, ec.PSNR] == np.inf and ref[v, 1, 0] == np.inf and ref[v, 0, 0] == np.inf
                seen["empty"] += 1
            if fam == "black_gt":
                assert np.isnan(rows[v, ec.DEPTH_L1]) and np.isnan(rows[v, ec.DEPTH_RMSE]) and rows[v, ec.DEPTH_COUNT] == 0.0
                assert np.isnan(ref[v, 0, 4]) and np.isnan(ref[v, 1, 4])
                seen["novalid"] += 1
    assert all(n > 0 for n in seen.values()), seen


def test_without_depth_the_depth_entries_are_nan(eval_harness):
    b = ec.make_batch((5, 17, 33), 0, "none")
    rows, summary = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"])
    full, _ = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"], b["depth"], b["gt_depth"])
    assert np.isnan(rows[:, [ec.DEPTH_L1, ec.DEPTH_RMSE, ec.DEPTH_COUNT]]).all()
    assert np.array_equal(rows[:, [0, 1, 4, 5, 6]].view(np.uint32), full[:, [0, 1, 4, 5, 6]].view(np.uint32))
    assert np.isnan(summary[3]) and np.isnan(summary[4]) and np.isfinite(summary[1])


def test_bytes_are_torchs_division(eval_harness):
    torch = pytest.importorskip("torch")
    table = np.zeros(256, np.float32)
    eval_harness.fre_byte_table(table.ctypes.data)
    want = (torch.arange(256, dtype=torch.uint8) / 255).numpy()
    assert want.dtype == np.float32 and np.array_equal(table.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(ec.u8_to_f32(np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1).repeat(3, -1))[0, 0, 0].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("kind", ec.MASK_KINDS)
def test_three_target_layouts_give_the_same_rows(eval_harness, kind):
    for shape in ec.SHAPES:
        b = ec.make_batch(shape, 2, kind)
        got = [ec.harness_metrics(eval_harness, b["render"], ec.target_of(b, lay), b["depth"], b["gt_depth"], b["mask"]) for lay in ec.LAYOUTS]
        for rows, summary in got[1:]:
            assert np.array_equal(rows.view(np.uint32), got[0][0].view(np.uint32))
            assert np.array_equal(summary.view(np.uint32), got[0][1].view(np.uint32))


def test_clamp_keeps_a_nan(eval_harness):
    f = eval_harness.fre_clamp_of
    assert f(-0.25) == 0.0 and f(1.5) == 1.0 and f(0.375) == 0.375 and f(0.0) == 0.0 and f(1.0) == 1.0
    assert np.isnan(f(float("nan"))) and f(float("inf")) == 1.0 and f(float("-inf")) == 0.0


def test_summary_follows_the_keep_rule(eval_harness):
    b = ec.make_batch((5, 17, 33), 0, "none")                # noise, smooth, step, identical, near
    assert b["families"][3] == "identical"
    rows, summary = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"], b["depth"], b["gt_depth"])
    want = ec.summary64(rows)
    assert summary[0] == 4.0 and summary[7] == 5.0 and summary[5] == 0.0 and summary[6] == 0.0
    assert np.array_equal(summary, want.astype(np.float32))          # float64 sums of 4 floats in index order: one rounding
    assert np.isclose(summary[1], rows[[0, 1, 2, 4], ec.PSNR].astype(np.float64).mean(), rtol=1e-7)
    # a NaN pixel in the render survives the clamp: that view's PSNR is NaN, it is KEPT and poisons the means
    bad = b["render"].copy()
    bad[1, 2, 3, 4] = np.nan
    rows_n, summary_n = ec.harness_metrics(eval_harness, bad, b["gt_f32"], b["depth"], b["gt_depth"])
    assert np.isnan(rows_n[1, ec.PSNR]) and np.isnan(rows_n[1, ec.SSIM]) and np.isfinite(rows_n[1, ec.DEPTH_L1])
    assert summary_n[0] == 4.0 and np.isnan(summary_n[1]) and np.isnan(summary_n[2]) and np.isfinite(summary_n[3])
    assert np.array_equal(np.delete(rows_n, 1, 0).view(np.uint32), np.delete(rows, 1, 0).view(np.uint32))
    # every view left out: a count of 0 and NaN means
    rows_e, summary_e = ec.harness_metrics(eval_harness, b["gt_f32"], b["gt_f32"], b["depth"], b["gt_depth"])
    assert np.all(rows_e[:, ec.PSNR] == np.inf) and summary_e[0] == 0.0 and summary_e[7] == 5.0 and np.isnan(summary_e[1:5]).all()
    # the summary alone over given rows, -inf left out as torch.isinf leaves it out
    r = np.zeros((4, ec.ROW), np.float32)
    r[:, 0], r[:, 1], r[:, 2], r[:, 3] = [30.0, -np.inf, 20.0, np.inf], [0.5, 0.1, 0.7, 1.0], [0.1, 9.0, 0.3, 0.0], [0.2, 9.0, 0.4, 0.0]
    s = ec.harness_summary(eval_harness, r)
    assert np.array_equal(s, ec.summary64(r).astype(np.float32))
    assert s[0] == 2.0 and s[1] == 25.0 and s[7] == 4.0


# ---- the ABI, without a device ------------------------------------------------------------------------------------------------------

def test_names_are_declared_and_exported(lib):
    from fisher_rast import _lib
    hdr = open(os.path.join(ROOT, "include", "fisher_rast.h")).read()
    for name in ("fr_view_metrics_workspace_bytes", "fr_view_metrics"):
        assert name + "(" in hdr and name in _lib.EXPORTS and hasattr(lib, name)
    assert "FR_EVAL_ROW 8" in hdr and _lib.FR_EVAL_ROW == ec.ROW
    assert lib.fr_version() == 100


def test_workspace_query_is_host_only(lib):
    f = lib.fr_view_metrics_workspace_bytes
    assert f(0, 16, 16) == 0 and f(1, 0, 16) == 0 and f(1, 16, 0) == 0 and f(-1, 16, 16) == 0 and f(65536, 16, 16) == 0
    assert f(1, 16, 16) == 7 * 8 and f(1, 17, 33) == 7 * 8 * 6 and f(64, 256, 256) == 64 * 7 * 256 * 8
    sizes = [int(f(v, 48, 64)) for v in (1, 2, 5, 64, 2000)]
    assert sizes == sorted(sizes) and all(s % 8 == 0 for s in sizes)


def test_abi_rejections(lib):
    from fisher_rast import _lib
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    a += (-a) % 256
    V, H, W = 2, 17, 33
    need = int(lib.fr_view_metrics_workspace_bytes(V, H, W))
    ok_cfg = dict(V=V, H=H, W=W, gt_layout=_lib.FR_EVAL_GT_U8_HWC, gt_channels=4, clamp_render=1, depth_valid_only=0,
                  render_view_stride=3 * H * W, depth_view_stride=3 * H * W, gt_depth_view_stride=H * W)
    ok = dict(render=a, depth=a + 8, gt=a + 16, gt_depth=a + 24, mask=None, rows=a + 32, summary=a + 40, ws=a + 1024, ws_bytes=need)

    def call(cfg=None, null_cfg=False, **kw):
        c = _lib.ViewMetricsCfg(**{**ok_cfg, **(cfg or {})})
        p = {**ok, **kw}
        return lib.fr_view_metrics(None if null_cfg else ctypes.byref(c), p["render"], p["depth"], p["gt"], p["gt_depth"], p["mask"], p["rows"],
                                   p["summary"], p["ws"], p["ws_bytes"], None)
    bad_cfgs = [dict(V=0), dict(H=0), dict(W=-3), dict(V=65536), dict(gt_layout=2), dict(gt_layout=-1), dict(gt_channels=2), dict(gt_channels=5),
                dict(clamp_render=2), dict(depth_valid_only=-1), dict(render_view_stride=3 * H * W - 1), dict(depth_view_stride=H * W - 1),
                dict(gt_depth_view_stride=0)]
    for bad in bad_cfgs:
        assert call(cfg=bad) == _lib.FR_EINVAL, bad
        assert b"fr_view_metrics" in lib.fr_last_error()
    assert call(null_cfg=True) == _lib.FR_EINVAL
    for bad in (dict(render=None), dict(gt=None), dict(rows=None), dict(summary=None), dict(depth=None), dict(gt_depth=None), dict(ws=None),
                dict(ws=a + 1028), dict(ws_bytes=need - 1), dict(ws_bytes=0)):
        assert call(**bad) == _lib.FR_EINVAL, bad
        assert b"fr_view_metrics" in lib.fr_last_error()
    assert b"workspace" in lib.fr_last_error()
    # a float target ignores gt_channels; the strides of an absent depth are not looked at
    assert lib.fr_view_metrics_summary(None, 4, a, None) == _lib.FR_EINVAL and lib.fr_view_metrics_summary(a, 0, a + 64, None) == _lib.FR_EINVAL
    assert b"fr_view_metrics_summary" in lib.fr_last_error()


def test_view_metrics_rejects_what_it_cannot_take():
    torch = pytest.importorskip("torch")
    from fisher_rast import ops
    r, g = torch.zeros((2, 3, 8, 8)), torch.zeros((2, 3, 8, 8))
    with pytest.raises(ValueError):
        ops.view_metrics(r, g)                                       # not on a HIP device


def test_render_eval_ops_install_grafts_exactly_its_surface():
    from models.SLAM.gaussian import GaussianSLAM, RenderEvalOps, RenderOps
    from models.SLAM.gaussian_object import GaussianObjectSLAM

    class Target:
        pass
    before = set(vars(Target))
    assert RenderEvalOps.install(Target) is Target
    assert set(vars(Target)) - before == {"eval_views", "frame_metrics"}
    for name in ("eval_views", "frame_metrics"):
        assert getattr(Target, name) is getattr(RenderEvalOps, name)
        assert getattr(GaussianSLAM, name) is getattr(RenderEvalOps, name) and getattr(GaussianObjectSLAM, name) is getattr(RenderEvalOps, name)
    assert not {"eval_views", "frame_metrics"} & set(vars(RenderOps)) and "render_at_pose" not in vars(RenderEvalOps)


def test_evaluate_views_rejects_what_it_cannot_take():
    torch = pytest.importorskip("torch")
    from fisher_rast.render_eval import evaluate_views
    with pytest.raises(ValueError):
        evaluate_views(object(), torch.eye(4)[None], torch.zeros((1, 3, 8, 8)))          # neither a scorer nor a SLAM object


def test_calc_psnr_and_calc_mse_on_the_host():
    torch = pytest.importorskip("torch")
    from models.SLAM.utils.slam_external import calc_mse, calc_psnr
    g = torch.Generator().manual_seed(3)
    x, y = torch.rand((3, 9, 7), generator=g), torch.rand((3, 9, 7), generator=g)
    mse = ((x.double() - y.double()) ** 2).reshape(3, -1).mean(1, keepdim=True)
    assert calc_mse(x, y).shape == (3, 1) and torch.allclose(calc_mse(x, y).double(), mse, rtol=1e-6)
    assert calc_psnr(x, y).shape == (3, 1) and torch.allclose(calc_psnr(x, y).double(), 20 * torch.log10(1.0 / torch.sqrt(mse)), rtol=1e-6)
    assert torch.isinf(calc_psnr(x, x)).all()
