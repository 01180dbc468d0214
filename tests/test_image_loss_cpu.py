"""The fused image loss's arithmetic (csrc/fr_loss_math.h, compiled with g++ in tests/harness/fr_loss_harness.cpp) on the CPU,
against what the reference's own calc_ssim / calc_ssim_masked / calc_loss / calc_loss_mask gave in binary32 and binary64
(tests/golden/reference_loss.npz).  The rule: a result must be within 2 D_ref + 64 2^-24 scale of the reference's binary64 run,
D_ref = the deviation of the reference's own binary32 run from it (loss_cases.tolerance) -- the separable binary32 chain is another
rounding of the same statement and cannot be asked to sit closer to the exact value than the reference's does."""
import numpy as np
import pytest

import loss_cases as lc


@pytest.fixture(scope="module")
def loss_harness():
    return lc.build_harness()


@pytest.fixture(scope="module")
def fixture():
    return lc.load_fixture()


def _value(term, out):
    return out[2] if term.out == "ssim" else out[0]


def test_taps_are_the_references_bits(loss_harness, fixture):
    import ctypes
    got = (ctypes.c_float * 11)()
    loss_harness.frl_taps(got)
    bits = np.array(list(got), np.float32).view(np.uint32)
    assert np.array_equal(bits, fixture[1]) and np.array_equal(bits, lc.TAPS_BITS)
    assert len(set(bits.tolist())) == 6 and np.array_equal(bits, bits[::-1])


def test_fixture_covers_every_case(fixture):
    want = {lc.key(s, f, k, t.name) for s, f, k in lc.all_cases() for t in lc.terms_for(s[0], k)}
    assert set(fixture[0]) == want and len(want) == 165


@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_restatement_equals_the_references_binary64_run(fixture, shape):
    worst = 0.0
    for family in lc.FAMILIES:
        for kind in lc.MASK_KINDS:
            x, y, m1, mc = lc.make_case(shape, family, kind)
            for term in lc.terms_for(shape[0], kind):
                _, v64, _, g64 = fixture[0][lc.key(shape, family, kind, term.name)]
                out, grad = lc.loss64(x, y, term.pick_mask(m1, mc), term.w_l1, term.w_ssim, term.denom, term.weights_map)
                v = _value(term, out)
                if np.isnan(v64):
                    assert np.isnan(v), (family, kind, term.name)
                else:
                    assert abs(v - v64) <= 1e-12 * max(1.0, abs(v64)), (family, kind, term.name, v, v64)
                    worst = max(worst, abs(v - v64) / max(1.0, abs(v64)))
                if g64.size:            # stored as binary32: half an ulp of the largest entry is all the file can tell apart
                    assert np.abs(grad.reshape(-1) - g64).max() <= 2.0 ** -24 * max(np.abs(g64).max(), 1e-30) + 1e-12, (family, kind, term.name)
    print(f"restatement vs reference binary64, {shape}: worst relative value difference {worst:.2e}")


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_harness_against_the_reference_by_the_rule(loss_harness, fixture, shape, family):
    """Every mask kind and term of one (shape, family), loss and gradient, by the rule; prints the need (deviation / bound).

    The window moments are taken about 0.5 (fr_loss_math.h) for the sake of this rule: with raw moments `step` at 3x17x33 -- a
    target exactly constant on either side of the step, render noise of 1e-2, so sigma^2 ~ 1e-4 under c2 = 9e-4 -- missed it on
    the gradient (calc_ssim 4.88e-06 against a bound of 3.27e-06, mapping calc_loss 9.77e-07 against 5.40e-07), and the miss was
    the binary32 second moments alone (7.9e-07 with them in binary64, 3.9e-06 with everything else in binary64).  Measured need
    now, worst over the 20 groups: loss 0.12, gradient 0.49 (that group)."""
    n = shape[0] * shape[1] * shape[2]
    need = np.zeros(2)
    failures = []
    for kind in lc.MASK_KINDS:
        x, y, m1, mc = lc.make_case(shape, family, kind)
        for term in lc.terms_for(shape[0], kind):
            v32, v64, gdev, g64 = fixture[0][lc.key(shape, family, kind, term.name)]
            mask = term.pick_mask(m1, mc)
            if not g64.size:
                g64 = lc.loss64(x, y, mask, term.w_l1, term.w_ssim, term.denom, term.weights_map)[1].reshape(-1)
            fwd = lc.harness_forward(loss_harness, x, y, mask, term.w_l1, term.w_ssim, term.denom, term.weights_map)
            grad = lc.harness_backward(loss_harness, x, y, mask, term.w_ssim, fwd["saved"], 1.0, term.weights_map)
            v = float(np.float32(_value(term, fwd["out"])))
            assert not np.isnan(grad).any(), (kind, term.name)
            lneed, gneed = lc.needs(term, n, v, grad, v32, v64, g64, gdev)
            if np.isnan(v64):
                assert kind == "empty", (kind, term.name)
            need = np.maximum(need, [lneed, gneed])
            if lneed > 1.0 or gneed > 1.0:
                failures.append((kind, term.name, lneed, gneed))
    print(f"need (deviation / bound) {shape} {family:9s}: loss {need[0]:.3f}  gradient {need[1]:.3f}")
    assert not failures, failures


def test_empty_mask_gives_nan_mean_zero_gradient(loss_harness):
    x, y, m1, mc = lc.make_case((3, 17, 33), "noise", "empty")
    for mask, w_ssim in ((mc, 0.2), (mc, 0.0), (m1, 0.0)):
        fwd = lc.harness_forward(loss_harness, x, y, mask, 0.8, w_ssim, lc.L1_MASKED_MEAN)
        assert np.isnan(fwd["out"][0]) and np.isnan(fwd["out"][1]) and fwd["out"][3] == 0.0
        grad = lc.harness_backward(loss_harness, x, y, mask, w_ssim, fwd["saved"], 0.37)
        assert not np.isnan(grad).any() and not grad.any()
    # the masked SUM of nothing is 0, and calc_ssim_masked clamps its count to 1
    fwd = lc.harness_forward(loss_harness, x, y, mc, 1.0, 0.0, lc.L1_SUM)
    assert fwd["out"][0] == 0.0
    fwd = lc.harness_forward(loss_harness, x, y, m1, 0.0, -1.0, lc.L1_SUM, True)
    assert fwd["out"][2] == 0.0 and not lc.harness_backward(loss_harness, x, y, m1, -1.0, fwd["saved"], 1.0, True).any()


def test_sign_of_zero_is_zero_and_identical_images_have_no_gradient(loss_harness):
    assert loss_harness.frl_sign_of(0.0) == 0.0 and loss_harness.frl_sign_of(-0.0) == 0.0
    assert loss_harness.frl_sign_of(1e-30) == 1.0 and loss_harness.frl_sign_of(-1e-30) == -1.0
    x, y, _, _ = lc.make_case((3, 17, 33), "identical", "none")
    for w_l1, w_ssim, denom in ((1.0, 0.0, lc.L1_SUM), (0.8, 0.2, lc.L1_MEAN)):
        fwd = lc.harness_forward(loss_harness, x, y, None, w_l1, w_ssim, denom)
        assert fwd["out"][1] == 0.0
        assert not lc.harness_backward(loss_harness, x, y, None, w_ssim, fwd["saved"], 1.0).any()
    # render == target: every SSIM term is exactly 1 in binary32 (A1 = B1, A2 = B2 bit for bit)
    assert np.all(fwd["ssim_map"] == 1.0) and fwd["out"][2] == 1.0 and fwd["out"][0] == 0.0


def test_masked_l1_counts_only_the_masked_pixels(loss_harness):
    x, y, m1, mc = lc.make_case((3, 5, 70), "noise", "half")
    fwd = lc.harness_forward(loss_harness, x, y, mc, 1.0, 0.0, lc.L1_MASKED_MEAN)
    want = np.abs(x - y).astype(np.float64)[mc]
    assert fwd["out"][3] == mc.sum() and abs(fwd["out"][0] - want.mean()) <= 1e-12
    fwd1 = lc.harness_forward(loss_harness, x, y, m1, 1.0, 0.0, lc.L1_SUM)
    assert fwd1["out"][3] == 3 * m1.sum() and abs(fwd1["out"][0] - (np.abs(x - y).astype(np.float64) * m1).sum()) <= 1e-9


def test_install_hands_get_loss_the_fused_loss_only_when_asked(monkeypatch):
    """`fused_loss=True` swaps the loss function `make_get_loss` is built around -- calc_loss, or calc_loss_mask where the patched
    module has one -- and nothing else; the default keeps the module's own.  Without a GPU the loss functions raise (no fallback)."""
    import sys
    import types
    import torch
    from fisher_rast._lib import FisherRastError
    from models.SLAM import gaussian as G, gaussian_object as GO
    from models.SLAM.utils import slam_external as se, slam_helpers as sh
    monkeypatch.setattr(G, "make_get_loss", lambda transform, loss: ("made", transform, loss))
    mod = types.ModuleType("fake_ref_gaussian_loss")
    mod.get_loss, mod.transform_to_frame, mod.calc_loss = "reference", object(), object()
    sys.modules[mod.__name__] = mod
    try:
        cls = type("RefSLAM", (), {"__module__": mod.__name__})
        G.FisherOps.install(cls, fused_loss=True)
        assert mod.get_loss == "reference"
        G.FisherOps.install(cls, patch_get_loss=True)
        assert mod.get_loss == ("made", mod.transform_to_frame, mod.calc_loss)
        G.FisherOps.install(cls, patch_get_loss=True, fused_loss=True)
        assert mod.get_loss == ("made", mod.transform_to_frame, sh.calc_loss)
        mod.calc_loss_mask = object()
        GO.ObjectFisherOps.install(cls, patch_get_loss=True, fused_loss=True)
        assert mod.get_loss == ("made", mod.transform_to_frame, sh.calc_loss_mask)
    finally:
        del sys.modules[mod.__name__]
    x = torch.zeros((3, 12, 12))
    with pytest.raises(NotImplementedError):
        se.calc_ssim(x, x, window_size=7)
    with pytest.raises(FisherRastError):
        sh.calc_loss(dict(im=x, depth=x[:1]), x, x[:1], x[:1] > 0, x > 0, True, False, False, False)
