"""-m "not gpu": the object-aware training step (fr_loss_mask, fr_bg_penalty_forward / _backward, fr_outside_mask) below the kernels.

The g++ harness over csrc/fr_objloss_math.h -- the header the kernels compile -- against a NumPy binary32 restatement and the torch
chain on the CPU (mask: every pixel and the median's bits, exactly), against torch autograd (penalty gradients: bit for bit; values:
by the rule of tests/loss_cases.py), against torch's matmul chain (outside mask: every Gaussian and the status words on the exact
family; on a general camera every Gaussian outside a band around the decisions, which may hold 1 % of them at most) and against what
the reference's own get_loss / get_gaussians_outside_mask gave on the CPU (tests/golden/reference_object_loss.npz).  Then the host
logic of the flags."""
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

import objloss_cases as oc


@pytest.fixture(scope="module")
def h():
    return oc.build_harness()


@pytest.fixture(scope="module")
def golden():
    return oc.load_golden()


# ---- 1. the mask ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_harness_equals_numpy_and_the_torch_chain_on_every_pixel(h, shape):
    checked = 0
    for family in oc.MASK_FAMILIES:
        ds, gt = oc.make_mask_case(shape, family)
        for kind in oc.OBJ_KINDS:
            obj = oc.make_obj(shape, kind)
            for reject, presence in oc.FLAGS:
                tag = (shape, family, kind, reject, presence)
                mask, status = oc.harness_mask(h, ds, gt, oc.SIL_THRES, reject, presence, obj)
                want_np, bits_np = oc.mask_numpy(ds, gt, oc.SIL_THRES, reject, presence, obj)
                want_t, bits_t = oc.mask_torch(ds, gt, oc.SIL_THRES, reject, presence, obj)
                assert set(np.unique(mask)) <= {0, 1}, tag
                assert np.array_equal(mask.astype(bool), want_np), tag
                assert np.array_equal(mask.astype(bool), want_t), tag
                assert int(np.uint32(status[4])) == bits_np == bits_t, (tag, hex(int(np.uint32(status[4]))), hex(bits_np), hex(bits_t))
                assert status[0] == int(mask.sum()) and status[1] == int(bits_np == oc.NAN_BITS and reject) and status[3] == 0, tag
                assert status[2] == (0 if obj is None else int((obj == 0).sum())), tag
                checked += 1
    assert checked == len(oc.MASK_FAMILIES) * len(oc.OBJ_KINDS) * len(oc.FLAGS)


def test_mask_families_do_what_their_names_say(h):
    shape = (37, 53)
    n = shape[0] * shape[1]
    kept = lambda family, reject, presence: oc.harness_mask(h, *oc.make_mask_case(shape, family), oc.SIL_THRES, reject, presence, None)
    for family in ("nan_depth", "inf_depth"):
        mask, status = kept(family, True, False)
        assert status[1] == 1 and np.uint32(status[4]) == oc.NAN_BITS and not mask.any()             # a NaN median: nothing passes
        assert kept(family, False, False)[0].any()
    for family in ("gt_zero", "mostly_unmeasured"):
        mask, status = kept(family, True, False)
        assert status[4] == 0 and not mask.any()                                                    # median 0 and a strict `<`
    assert kept("mostly_unmeasured", False, False)[0].any()
    ds, gt = oc.make_mask_case(shape, "ten_med")
    mask, status = oc.harness_mask(h, ds, gt, oc.SIL_THRES, True, False, None)
    err = np.abs(gt[0] - ds[0])
    assert np.float32(0.125).view(np.uint32) == np.uint32(status[4]) and (err == 1.25).any() and not mask[err == 1.25].any() and mask[err == 1.0].all()
    ds, gt = oc.make_mask_case(shape, "plateau")
    assert np.uint32(oc.harness_mask(h, ds, gt, oc.SIL_THRES, True, False, None)[1][4]) == np.float32(0.5).view(np.uint32)
    ds, gt = oc.make_mask_case(shape, "sil_at_thres")
    mask, _ = oc.harness_mask(h, ds, gt, oc.SIL_THRES, False, True, None)
    at = ds[1] == np.float32(oc.SIL_THRES)
    assert at.any() and not mask[at].any() and mask[(ds[1] > np.float32(oc.SIL_THRES)) & (gt[0] > 0)].all()
    ds, gt = oc.make_mask_case(shape, "neg_zero_gt")
    assert np.signbit(gt[gt == 0]).any() and 0 < int(oc.harness_mask(h, ds, gt, oc.SIL_THRES, True, True, None)[0].sum()) < n
    ds, gt = oc.make_mask_case(shape, "half")
    for reject, presence in oc.FLAGS:
        share = oc.harness_mask(h, ds, gt, oc.SIL_THRES, reject, presence, oc.make_obj(shape, "half"))[0].mean()
        assert 0.005 < share < 0.5, (reject, presence, share)


# ---- 2. the penalties -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_penalty_values_by_the_rule_and_gradients_bit_for_bit(h, shape):
    worst = 0.0
    for family in oc.PENALTY_FAMILIES:
        for kind in oc.PENALTY_OBJ:
            tag = (shape, family, kind)
            im, ds, obj = oc.make_penalty_case(shape, family, kind)
            got = oc.harness_penalty(h, im, ds, obj)
            v32, g_im32, g_ds32 = oc.penalty_torch(im, ds, obj, torch.float32)
            v64, _, _ = oc.penalty_torch(im, ds, obj, torch.float64)
            need = oc.value_need(got["out4"][0], v32, v64)
            worst = max(worst, need)
            assert need <= 1.0, (tag, got["out4"], v32, v64)
            n = int((obj == 0).sum())
            assert got["out4"][3] == n and got["saved2"][0] == max(3 * n, 1) and got["saved2"][1] == max(n, 1), tag
            assert oc.same_bits(got["g_im"], g_im32), (tag, np.flatnonzero(got["g_im"].view(np.uint32) != g_im32.view(np.uint32))[:4])
            assert oc.same_bits(got["g_ds"], g_ds32), (tag, np.flatnonzero(got["g_ds"].view(np.uint32) != g_ds32.view(np.uint32))[:4])
            assert not got["g_ds"][0].any() and not got["g_ds"][2].any(), tag
            if kind == "ones":                                                  # no background: denominators 1, nothing but zeros
                assert not got["g_im"].any() and not got["g_ds"].any(), tag
            if family in ("nan_inside", "nan_outside"):
                assert np.isnan(got["out4"][1]) and np.isnan(got["out4"][0]), tag
            if family == "sil_nan":
                assert np.isnan(got["out4"][2]) and not np.isnan(got["out4"][1]), tag
            if family == "sil_inf":
                assert np.isfinite(got["out4"]).all(), tag
    print(f"penalty {shape}: largest need (deviation / bound) {worst:.3f}")


# ---- 3. the outside mask ----------------------------------------------------------------------------------------------------------------

def _exact_case(P, shape, cols, seed=0):
    case = oc.make_outside_case(P, shape, cols, "exact", seed)
    case["logs"] = np.where(oc.exp_is_correctly_rounded(case["logs"]), case["logs"], np.float32(0.0)).astype(np.float32)
    return case


@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("shape", oc.OUTSIDE_MASKS, ids=lambda s: "x".join(map(str, s)))
def test_outside_mask_exact_family_equals_torch_on_every_gaussian(h, shape, cols):
    for P in oc.OUTSIDE_P:
        for seed in (0, 1):
            case = _exact_case(P, shape, cols, seed)
            outside, status = oc.harness_outside(h, case)
            want = oc.outside_torch(case, torch.float32)
            assert np.array_equal(outside.astype(bool), want["outside"]), (P, seed, int((outside.astype(bool) != want["outside"]).sum()))
            assert np.array_equal(status.view(np.uint32).astype(np.int64), want["status"]), (P, seed, status, want["status"])
    # P = 4096 has Gaussians on both sides; a NaN scale on one side makes that side's range NaN and leaves the other
    case = _exact_case(4096, shape, cols)
    outside, status = oc.harness_outside(h, case)
    assert 0 < status[0] < 4096 and status[0] + status[1] == 4096
    first_inside = int(np.flatnonzero(outside == 0)[0])
    case["logs"][first_inside, cols - 1] = np.nan
    outside2, status2 = oc.harness_outside(h, case)
    want = oc.outside_torch(case, torch.float32)
    assert np.array_equal(outside, outside2) and np.array_equal(status2.view(np.uint32).astype(np.int64), want["status"])
    assert np.uint32(status2[2]) == np.uint32(status2[3]) == oc.NAN_BITS and np.array_equal(status2[4:], status[4:])


@pytest.mark.parametrize("P,shape", [(4096, (48, 64)), (20000, (37, 53))], ids=["4096-48x64", "20000-37x53"])
def test_outside_mask_general_camera_against_binary64(h, P, shape):
    case = oc.make_outside_case(P, shape, 3, "general")
    outside, status = oc.harness_outside(h, case)
    want = oc.outside_torch(case, torch.float64)
    ref32 = oc.outside_torch(case, torch.float32)
    band = oc.outside_band(want["u"], want["v"], want["z"], shape[1], shape[0])
    share = float(band.mean())
    print(f"outside mask {P} / {shape}: {100 * share:.2f} % of the Gaussians in the band, inside {int(status[0])}")
    assert share <= 0.01
    assert np.array_equal(outside.astype(bool)[~band], want["outside"][~band])
    assert np.array_equal(ref32["outside"][~band], want["outside"][~band])
    assert status[0] + status[1] == P and status[0] == int((outside == 0).sum()) and status[0] > 0


# ---- 4. against the reference's own runs ------------------------------------------------------------------------------------------------

def _get_loss_on_the_cpu(monkeypatch, case, mode, **flags):
    """make_get_loss around a render that hands back the case's images as leaves (what the golden script gave the reference)"""
    import models.SLAM.gaussian as G
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    im, ds = t(case["im"]).clone().requires_grad_(True), t(case["depth_sil"]).clone().requires_grad_(True)
    seen = {}
    monkeypatch.setattr(G, "render_rgb_depth_sil", lambda params, cam, w2c, pts, **k: (im, torch.arange(7) % 3, ds, dict(means2D=torch.zeros(7, 3))))
    monkeypatch.setattr(G, "update_seen_and_radius", lambda variables, radius: variables)
    inner = oc.torch_calc_loss(masked_mapping=True)

    def calc(curr, im_, depth_, mask, color_mask, *f):
        seen["mask"] = mask.detach().clone()
        return inner(curr, im_, depth_, mask, color_mask, *f)

    curr = dict(cam=None, w2c=torch.eye(4), im=t(case["gt_im"]), depth=t(case["gt"]))
    if "obj" in case:
        curr["obj_mask_2d"] = case["obj"] if (case["obj"] is None or torch.is_tensor(case["obj"])) else t(case["obj"]).bool()
    loss, _, weighted = G.make_get_loss(lambda *a, **k: None, calc, **flags)(
        {}, curr, {}, 0, oc.GOLDEN_WEIGHTS, True, oc.SIL_THRES, True, case["ignore"], tracking=mode == "tracking", mapping=mode == "mapping")
    loss.backward()
    return dict(weighted=np.array([float(weighted[k].detach()) for k in ("im", "depth", "loss")], np.float32), mask=seen["mask"][0].numpy(),
                d_im=im.grad.numpy(), d_depth_sil=ds.grad.numpy())


@pytest.mark.parametrize("mode", ["tracking", "mapping"])
@pytest.mark.parametrize("i", range(len(oc.GOLDEN_LOSS_CASES)))
def test_object_get_loss_reproduces_the_reference(monkeypatch, golden, i, mode):
    """The torch route of make_get_loss(object_mask=True) on the CPU against the reference's get_loss of the object class: the mask,
    the depth term (which depends on the mask alone) and the gradients' zero pattern exactly, the values and the gradients by the
    rule.  Without the object lines (object_mask=False: all the parent commit has) the loss is another one."""
    case, run = oc.make_golden_loss_case(i), f"loss/{i}/{mode}"
    got = _get_loss_on_the_cpu(monkeypatch, case, mode, object_mask=True)
    assert np.array_equal(got["mask"], golden[f"{run}/mask"])
    assert got["weighted"][1] == golden[f"{run}/weighted"][1]
    for k in range(3):
        need = oc.value_need(got["weighted"][k], golden[f"{run}/weighted"][k], golden[f"{run}/weighted64"][k])
        assert need <= 1.0, (k, got["weighted"], golden[f"{run}/weighted"], golden[f"{run}/weighted64"])
    for name in ("d_im", "d_depth_sil"):
        assert np.array_equal(got[name] == 0, golden[f"{run}/{name}"] == 0), name
        assert oc.grad_need(got[name], golden[f"{run}/{name}"], golden[f"{run}/{name}64"]) <= 1.0, name
    plain = _get_loss_on_the_cpu(monkeypatch, case, mode)
    assert oc.value_need(plain["weighted"][2], golden[f"{run}/weighted"][2], golden[f"{run}/weighted64"][2]) > 1.0
    assert not np.array_equal(plain["mask"], golden[f"{run}/mask"])


@pytest.mark.parametrize("i", range(len(oc.GOLDEN_OUTSIDE_CASES)))
def test_outside_mask_against_the_reference(h, golden, i):
    from models.SLAM.gaussian import frame_w2c
    case = oc.make_golden_outside_case(i)
    params = oc.trajectory_params(case, t=oc.GOLDEN_FRAME)
    case["w2c"] = frame_w2c(params, oc.GOLDEN_FRAME).numpy().astype(np.float32)            # the pose the product derives from the trajectory
    outside, status = oc.harness_outside(h, case)
    ref64 = dict(case, w2c=np.eye(4))
    ref64["w2c"][:3, :3] = oc.rotation_of(case["quat"].astype(np.float64))
    ref64["w2c"][:3, 3] = case["w2c"][:3, 3]
    want = oc.outside_torch(dict(ref64, means=case["means"], K=case["K"]), torch.float64)
    H, W = case["obj"].shape
    band = oc.outside_band(want["u"], want["v"], want["z"], W, H)
    assert int(band.sum()) <= -(-len(band) // 100)                                 # 1 % of the Gaussians, rounded up to a whole one
    gold = golden[f"outside/{i}/outside"]
    assert np.array_equal(outside.astype(bool)[~band], gold[~band]) and np.array_equal(want["outside"][~band], gold[~band])
    counts = golden[f"outside/{i}/counts"]
    assert abs(int(status[0]) - int(counts[0])) <= int(band.sum()) and status[0] + status[1] == counts[2]
    if np.array_equal(outside.astype(bool), gold):
        assert np.allclose(status[2:].view(np.float32), golden[f"outside/{i}/ranges"], rtol=2e-7, atol=0)


# ---- 5. host logic ----------------------------------------------------------------------------------------------------------------------

def test_flags_are_off_by_default():
    import models.SLAM.gaussian as G
    import models.SLAM.gaussian_object as GO
    for fn in (G.make_get_loss, G.FisherOps.install, GO.ObjectFisherOps.install):
        p = inspect.signature(fn).parameters
        assert p["fused_mask"].default is False and p["object_mask"].default is False, fn
    assert inspect.signature(G.MapEditOps.install).parameters["outside_mask"].default == "module"


def test_install_passes_the_keywords_only_when_set(monkeypatch):
    import models.SLAM.gaussian as G
    import models.SLAM.gaussian_object as GO
    made = []
    monkeypatch.setattr(G, "make_get_loss", lambda transform, loss, **kw: made.append(kw) or "made")
    mod = types.ModuleType("objloss_fake_reference_module")
    mod.get_loss, mod.transform_to_frame, mod.calc_loss = "theirs", object(), object()
    monkeypatch.setitem(sys.modules, mod.__name__, mod)
    for ops in (G.FisherOps, GO.ObjectFisherOps):
        cls = type("Fake", (), {"__module__": mod.__name__})
        ops.install(cls, patch_get_loss=True)
        ops.install(cls, patch_get_loss=True, object_mask=True)
        ops.install(cls, patch_get_loss=True, fused_mask=True)
        ops.install(cls, patch_get_loss=True, fused_rendervar=True, fused_mask=True, object_mask=True)
        mod.get_loss = "theirs"
        ops.install(cls, fused_mask=True, object_mask=True)                     # without patch_get_loss nothing is replaced
        assert mod.get_loss == "theirs"
    assert made == [{}, {"object_mask": True}, {"fused_mask": True}, {"fused_rendervar": True, "fused_mask": True, "object_mask": True}] * 2
    # a two-argument stand-in keeps working while no flag is set
    monkeypatch.setattr(G, "make_get_loss", lambda transform, loss: "two")
    G.FisherOps.install(type("Fake", (), {"__module__": mod.__name__}), patch_get_loss=True)
    assert mod.get_loss == "two"


@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_object_mask_without_a_mask_is_the_plain_step_and_unsupported_inputs_take_the_torch_route(monkeypatch, mode):
    from fisher_rast import object_loss as ol
    case = oc.make_golden_loss_case(1)
    want = _get_loss_on_the_cpu(monkeypatch, {k: v for k, v in case.items() if k != "obj"}, mode)
    for missing in ({k: v for k, v in case.items() if k != "obj"}, dict(case, obj=None)):
        got = _get_loss_on_the_cpu(monkeypatch, missing, mode, object_mask=True)
        assert all(oc.same_bits(got[k], want[k]) for k in want)
    # CPU tensors are not what the kernels take: every fused call is refused before a launch, and the step is the torch route's
    monkeypatch.setattr(ol, "loss_mask_raw", lambda *a, **k: pytest.fail("a launch on unsupported inputs"))
    monkeypatch.setattr(ol, "penalty_forward_raw", lambda *a, **k: pytest.fail("a launch on unsupported inputs"))
    for flags in (dict(object_mask=True), dict()):
        torch_route = _get_loss_on_the_cpu(monkeypatch, case, mode, **flags)
        fused = _get_loss_on_the_cpu(monkeypatch, case, mode, fused_mask=True, **flags)
        assert all(oc.same_bits(fused[k], torch_route[k]) for k in fused), flags
    masked, plain = _get_loss_on_the_cpu(monkeypatch, case, mode, object_mask=True), _get_loss_on_the_cpu(monkeypatch, case, mode)
    assert masked["weighted"][2] != plain["weighted"][2] and not np.array_equal(masked["mask"], plain["mask"])


def test_unsupported_inputs_raise_before_any_launch(monkeypatch):
    from fisher_rast import _lib, object_loss as ol
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("the library was reached"))
    ds, gt = (torch.from_numpy(a) for a in oc.make_mask_case((5, 7), "half"))
    im = torch.zeros(3, 5, 7)
    obj = torch.ones(5, 7, dtype=torch.bool)
    params = dict(means3D=torch.zeros(4, 3), log_scales=torch.zeros(4, 3))
    for bad in (lambda: ol.loss_pixel_mask(ds, gt, 0.5, True, True),                               # not on a HIP device
                lambda: ol.loss_pixel_mask(ds.double(), gt, 0.5, True, True),
                lambda: ol.loss_pixel_mask(ds.permute(0, 2, 1), gt, 0.5, False, False),
                lambda: ol.loss_pixel_mask(ds[:2], gt, 0.5, False, False),
                lambda: ol.background_penalty(im, ds, obj),
                lambda: ol.background_penalty(im.double(), ds, obj),
                lambda: ol.outside_mask(params, torch.eye(4), torch.eye(3), obj),
                lambda: ol.outside_mask(dict(params, log_scales=torch.zeros(4, 2)), torch.eye(4), torch.eye(3), obj)):
        with pytest.raises(ol.ObjectLossUnsupported):
            bad()
    assert issubclass(ol.ObjectLossUnsupported, _lib.FisherRastError)
    # the layouts of an object mask
    want = oc.make_obj((5, 7), "half")
    for form in oc.OBJ_FORMS:
        m = ol.mask_bytes(oc.obj_form(want, form), 5, 7, torch.device("cpu"))
        assert m.dtype == torch.uint8 and m.shape == (5, 7) and np.array_equal(m.numpy() != 0, want != 0), form
    b = torch.from_numpy(want).bool()
    assert ol.mask_bytes(b, 5, 7, b.device).data_ptr() == b.data_ptr()                             # reinterpreted, not copied
    assert ol.mask_bytes(None, 5, 7, b.device) is None
    with pytest.raises(ol.ObjectLossUnsupported):
        ol.mask_bytes(b, 7, 5, b.device)


def test_get_gaussians_outside_mask_keeps_the_reference_return(h, golden, monkeypatch):
    from fisher_rast import object_loss as ol
    from models.SLAM.utils import slam_external as se
    case = oc.make_golden_outside_case(1)
    reads = []

    def on_the_harness(params, w2c, intrinsics, obj_mask):
        c = dict(case, w2c=np.ascontiguousarray(w2c.numpy(), np.float32), K=np.ascontiguousarray(intrinsics.numpy(), np.float32))
        outside, status = oc.harness_outside(h, c)
        st = torch.from_numpy(status)
        st.cpu = lambda: reads.append(1) or torch.from_numpy(status)
        return torch.from_numpy(outside).bool(), st

    monkeypatch.setattr(ol, "outside_mask", on_the_harness)
    params = oc.trajectory_params(case, t=oc.GOLDEN_FRAME)
    curr = dict(id=oc.GOLDEN_FRAME, intrinsics=torch.from_numpy(case["K"]))
    outside, stats = se.get_gaussians_outside_mask(params, curr, torch.from_numpy(case["obj"]).bool())
    assert list(stats) == ['in_count', 'out_count', 'total', 'inside_scale_min', 'inside_scale_max', 'outside_scale_min', 'outside_scale_max',
                           'idx_in', 'idx_out']                                      # the reference's keys, in its order
    assert outside.dtype == torch.bool and stats['total'] == 65 and stats['in_count'] + stats['out_count'] == 65
    assert torch.equal(stats['idx_out'], torch.nonzero(outside).squeeze(1)) and torch.equal(stats['idx_in'], torch.nonzero(~outside).squeeze(1))
    assert all(isinstance(stats[k], float) for k in ('inside_scale_min', 'inside_scale_max', 'outside_scale_min', 'outside_scale_max'))
    assert np.array_equal(outside.numpy(), golden["outside/1/outside"])
    assert [stats['in_count'], stats['out_count'], stats['total']] == golden["outside/1/counts"].tolist()
    assert np.allclose([stats[k] for k in ('inside_scale_min', 'inside_scale_max', 'outside_scale_min', 'outside_scale_max')],
                       golden["outside/1/ranges"], rtol=2e-7, atol=0)
    assert len(reads) == 1
    _, lean = se.get_gaussians_outside_mask(params, curr, torch.from_numpy(case["obj"]).bool(), with_indices=False)
    assert 'idx_in' not in lean and 'idx_out' not in lean and {k: v for k, v in stats.items() if not k.startswith('idx')} == lean
    assert len(reads) == 2


def test_map_edit_install_takes_the_library_outside_mask_when_asked(monkeypatch):
    import models.SLAM.gaussian as G
    from models.SLAM.utils import slam_external as se
    theirs = lambda params, curr_data, obj_mask_2d: None
    mod = types.ModuleType("objloss_fake_edit_module")
    mod.prune_gaussians = mod.densify = mod.remove_points = "theirs"
    mod.get_gaussians_outside_mask = theirs
    monkeypatch.setitem(sys.modules, mod.__name__, mod)
    cls = type("Fake", (), {"__module__": mod.__name__})
    G.MapEditOps.install(cls)
    assert mod.prune_gaussians.__self__.outside_mask_fn is theirs
    G.MapEditOps.install(cls, outside_mask="library")
    assert mod.prune_gaussians.__self__.outside_mask_fn is se.get_gaussians_outside_mask and mod.get_gaussians_outside_mask is theirs
    assert mod.densify.__self__ is mod.prune_gaussians.__self__ is mod.remove_points.__self__
    with pytest.raises(ValueError):
        G.MapEditOps.install(cls, outside_mask="torch")


def test_abi_is_declared_exported_and_mirrored():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    lib = _lib.load()
    header = open(next(h for h in _lib.HEADERS if h.endswith("fisher_rast.h"))).read()
    for name in ("fr_loss_mask_workspace_bytes", "fr_loss_mask", "fr_bg_penalty_workspace_bytes", "fr_bg_penalty_forward", "fr_bg_penalty_backward",
                 "fr_outside_mask_workspace_bytes", "fr_outside_mask"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f" {name}(" in header, name
    assert os.path.join(_lib._CSRC, "fr_objloss.hip") in _lib.UNITS and os.path.join(_lib._CSRC, "fr_objloss_math.h") in _lib.SOURCES
    assert f"#define FR_LOSS_MASK_STATUS_WORDS {_lib.FR_LOSS_MASK_STATUS_WORDS}" in header
    assert f"#define FR_OUTSIDE_STATUS_WORDS {_lib.FR_OUTSIDE_STATUS_WORDS}" in header
    assert lib.fr_loss_mask_workspace_bytes(0, 5) == 0 and lib.fr_loss_mask_workspace_bytes(5, 7) >= 4 * 256 * 4 + 4
    assert lib.fr_bg_penalty_workspace_bytes(64, 65) == 3 * 5 * 8 and lib.fr_outside_mask_workspace_bytes(4097) == 5 * 32
    # bad arguments are refused on the host, before anything is launched
    cfg = _lib.LossMaskCfg(0, 7, 0.5, 0, 10.0, 0)
    import ctypes
    assert lib.fr_loss_mask(ctypes.byref(cfg), None, None, None, None, None, None, 0, None) == _lib.FR_EINVAL
    assert lib.fr_bg_penalty_forward(5, 7, 0.1, 0.1, None, None, None, None, None, None, 0, None) == _lib.FR_EINVAL
    assert lib.fr_outside_mask(4, 2, None, None, None, None, None, 5, 7, None, None, None, 0, None) == _lib.FR_EINVAL
