"""-m gpu: the object-aware training step on the device (fr_loss_mask, fr_bg_penalty_forward / _backward, fr_outside_mask,
csrc/fr_objloss.hip) and what is written on it (fisher_rast/object_loss.py, make_get_loss(fused_mask=, object_mask=),
get_gaussians_outside_mask of models/SLAM/utils/slam_external.py).

Bit for bit against the g++ harness over the same header (tests/harness/fr_objloss_harness.cpp) for every family and shape of
tests/objloss_cases.py, on guarded buffers, twice; on a non-default stream in stream order; without a host synchronisation; inside
`make_get_loss` against the torch route and against the reference's own runs (tests/golden/reference_object_loss.npz)."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import objloss_cases as oc
import stream_cases as sc
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes behind every output
GUARD_BYTE = 0x5A


@pytest.fixture(scope="module")
def h():
    return oc.build_harness()


@pytest.fixture(scope="module")
def golden():
    return oc.load_golden()


class _Guarded:
    """a device buffer of `count` elements of `dtype` with GUARD bytes behind it"""

    def __init__(self, count, dtype, dev):
        self.nbytes = count * np.dtype(dtype).itemsize
        self.buf = torch.full((self.nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.dtype = dtype

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        return self.buf[:self.nbytes].cpu().numpy().view(self.dtype).copy()

    def intact(self):
        return bool((self.buf[self.nbytes:] == GUARD_BYTE).all())


def _dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _abi_mask(dev, ds, gt, reject, presence, obj):
    from fisher_rast import _lib
    lib = _lib.load()
    H, W = ds.shape[1:]
    dst, gtt, objt = _dev(ds, dev), _dev(gt, dev), _dev(obj, dev)
    nws = int(lib.fr_loss_mask_workspace_bytes(H, W))
    assert nws % 8 == 0 and nws >= 4 * 256 * 4 + 4
    mask, status, ws = _Guarded(H * W, np.uint8, dev), _Guarded(5, np.int32, dev), _Guarded(nws, np.uint8, dev)
    cfg = _lib.LossMaskCfg(H, W, oc.SIL_THRES, int(reject), oc.RATIO, int(presence))
    _lib.check(lib.fr_loss_mask(ctypes.byref(cfg), dst.data_ptr(), gtt.data_ptr(), _ptr(objt), mask.ptr, status.ptr, ws.ptr if reject else None,
                                nws if reject else 0, _stream(dev)), "fr_loss_mask")
    torch.cuda.synchronize()
    return mask.get().reshape(H, W), status.get(), all(g.intact() for g in (mask, status, ws))


def _abi_penalty(dev, im, ds, obj):
    from fisher_rast import _lib
    lib = _lib.load()
    H, W = obj.shape
    imt, dst, objt = _dev(im, dev), _dev(ds, dev), _dev(obj, dev)
    nws = int(lib.fr_bg_penalty_workspace_bytes(H, W))
    assert nws % 8 == 0 and nws > 0
    out4, saved2, ws = _Guarded(4, np.float32, dev), _Guarded(2, np.float32, dev), _Guarded(nws, np.uint8, dev)
    g_im, g_ds = _Guarded(3 * H * W, np.float32, dev), _Guarded(3 * H * W, np.float32, dev)
    up = torch.tensor([oc.UPSTREAM], dtype=torch.float32, device=dev)
    _lib.check(lib.fr_bg_penalty_forward(H, W, oc.LAMBDA, oc.LAMBDA, imt.data_ptr(), dst.data_ptr(), objt.data_ptr(), out4.ptr, saved2.ptr, ws.ptr, nws,
                                         _stream(dev)), "fr_bg_penalty_forward")
    _lib.check(lib.fr_bg_penalty_backward(H, W, oc.LAMBDA, oc.LAMBDA, imt.data_ptr(), dst.data_ptr(), objt.data_ptr(), saved2.ptr, up.data_ptr(), g_im.ptr,
                                          g_ds.ptr, _stream(dev)), "fr_bg_penalty_backward")
    torch.cuda.synchronize()
    res = dict(out4=out4.get(), saved2=saved2.get(), g_im=g_im.get().reshape(3, H, W), g_ds=g_ds.get().reshape(3, H, W))
    return res, all(g.intact() for g in (out4, saved2, ws, g_im, g_ds))


def _abi_outside(dev, case):
    from fisher_rast import _lib
    lib = _lib.load()
    P, cols = case["logs"].shape
    H, W = case["obj"].shape
    t = {k: _dev(case[k], dev) for k in ("means", "logs", "w2c", "K", "obj")}
    nws = int(lib.fr_outside_mask_workspace_bytes(P))
    assert nws % 8 == 0 and nws >= 32
    outside, status, ws = _Guarded(P, np.uint8, dev), _Guarded(6, np.int32, dev), _Guarded(nws, np.uint8, dev)
    _lib.check(lib.fr_outside_mask(P, cols, t["means"].data_ptr(), t["logs"].data_ptr(), t["w2c"].data_ptr(), t["K"].data_ptr(), t["obj"].data_ptr(), H, W,
                                   outside.ptr, status.ptr, ws.ptr, nws, _stream(dev)), "fr_outside_mask")
    torch.cuda.synchronize()
    return outside.get(), status.get(), all(g.intact() for g in (outside, status, ws))


# ---- 1. the ABI on guarded buffers ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", oc.SHAPES + [oc.GPU_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_loss_mask_is_the_harness_bit_for_bit(gpu, h, shape):
    families = oc.MASK_FAMILIES if shape in oc.SHAPES else ["half", "plateau"]
    for family in families:
        ds, gt = oc.make_mask_case(shape, family)
        for kind in oc.OBJ_KINDS:
            obj = oc.make_obj(shape, kind)
            for reject, presence in oc.FLAGS:
                tag = (shape, family, kind, reject, presence)
                want_mask, want_status = oc.harness_mask(h, ds, gt, oc.SIL_THRES, reject, presence, obj)
                mask, status, intact = _abi_mask(gpu, ds, gt, reject, presence, obj)
                assert intact, tag
                assert np.array_equal(mask, want_mask), (tag, int((mask != want_mask).sum()))
                assert np.array_equal(status, want_status), (tag, status, want_status)
                if family == families[0]:
                    mask2, status2, _ = _abi_mask(gpu, ds, gt, reject, presence, obj)
                    assert np.array_equal(mask, mask2) and np.array_equal(status, status2), tag


@pytest.mark.parametrize("shape", oc.SHAPES + [oc.GPU_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_background_penalty_is_the_harness_bit_for_bit(gpu, h, shape):
    families = oc.PENALTY_FAMILIES if shape in oc.SHAPES else ["plain", "sil_edges"]
    for family in families:
        for kind in oc.PENALTY_OBJ:
            tag = (shape, family, kind)
            im, ds, obj = oc.make_penalty_case(shape, family, kind)
            want = oc.harness_penalty(h, im, ds, obj)
            got, intact = _abi_penalty(gpu, im, ds, obj)
            assert intact, tag
            for k in want:
                assert oc.same_bits(got[k], want[k]), (tag, k, got[k].reshape(-1)[:4], want[k].reshape(-1)[:4])
            if family == families[0]:
                again, _ = _abi_penalty(gpu, im, ds, obj)
                assert all(oc.same_bits(got[k], again[k]) for k in got), tag


@pytest.mark.parametrize("cols", [1, 3])
@pytest.mark.parametrize("shape", oc.OUTSIDE_MASKS, ids=lambda s: "x".join(map(str, s)))
def test_outside_mask_is_the_harness_bit_for_bit(gpu, h, shape, cols):
    for family in ("exact", "general"):
        for P in oc.OUTSIDE_P:
            case = oc.make_outside_case(P, shape, cols, family)
            if P == 4096:
                case["logs"][17, cols - 1] = np.nan                      # a NaN scale: its side's range is NaN
            tag = (family, P, shape, cols)
            want_outside, want_status = oc.harness_outside(h, case)
            outside, status, intact = _abi_outside(gpu, case)
            assert intact, tag
            assert np.array_equal(outside, want_outside), (tag, int((outside != want_outside).sum()))
            assert np.array_equal(status, want_status), (tag, status.view(np.uint32), want_status.view(np.uint32))
            outside2, status2, _ = _abi_outside(gpu, case)
            assert np.array_equal(outside, outside2) and np.array_equal(status, status2), tag
    # no Gaussians at all: counts 0, every range NaN
    empty = dict(oc.make_outside_case(1, shape, cols, "exact"))
    empty["means"], empty["logs"] = np.zeros((0, 3), np.float32), np.zeros((0, cols), np.float32)
    from fisher_rast import _lib
    lib = _lib.load()
    t = {k: _dev(empty[k], gpu) for k in ("w2c", "K", "obj")}
    status, ws = _Guarded(6, np.int32, gpu), _Guarded(64, np.uint8, gpu)
    _lib.check(lib.fr_outside_mask(0, cols, None, None, t["w2c"].data_ptr(), t["K"].data_ptr(), t["obj"].data_ptr(), shape[0], shape[1], None,
                                   status.ptr, ws.ptr, 64, _stream(gpu)), "fr_outside_mask")
    torch.cuda.synchronize()
    assert status.get().view(np.uint32).tolist() == [0, 0] + [oc.NAN_BITS] * 4 and status.intact()


# ---- 2. a non-default stream, in stream order -------------------------------------------------------------------------------------------

def _stream_cases():
    shape = (37, 53)

    def make_mask(which):
        ds, gt = oc.make_mask_case(shape, ["half", "plateau"][which])
        return dict(ds=ds, gt=gt, obj=oc.make_obj(shape, "half", seed=which))

    def call_mask(ctx, b):
        from fisher_rast import object_loss as ol
        out = {}
        for reject in (False, True):
            mask, status = ol.loss_mask_raw(b["ds"], b["gt"], oc.SIL_THRES, reject, True, b["obj"])
            out[f"mask{int(reject)}"], out[f"status{int(reject)}"] = mask, status
        return out

    def make_penalty(which):
        im, ds, obj = oc.make_penalty_case(shape, ["plain", "sil_edges"][which], "half")
        return dict(im=im, ds=ds, obj=obj if which == 0 else oc.make_obj(shape, "half", seed=9))

    def call_penalty(ctx, b):
        from fisher_rast import object_loss as ol
        im, ds = b["im"].detach().requires_grad_(True), b["ds"].detach().requires_grad_(True)
        v = ol.background_penalty(im, ds, b["obj"])
        (v * oc.UPSTREAM).backward()
        return dict(value=v.detach().reshape(1), g_im=im.grad, g_ds=ds.grad)

    def make_outside(which):
        c = oc.make_outside_case(4096, shape, 3, "general", seed=which)
        return dict(means=c["means"], logs=c["logs"], w2c=c["w2c"], K=c["K"], obj=c["obj"])

    def call_outside(ctx, b):
        from fisher_rast import object_loss as ol
        outside, status = ol.outside_mask(dict(means3D=b["means"], log_scales=b["logs"]), b["w2c"], b["K"], b["obj"])
        return dict(outside=outside, status=status)

    return [sc.Case(name="loss_mask", make=make_mask, call=call_mask, exact=("mask0", "status0", "mask1", "status1"), sync_free=True),
            sc.Case(name="bg_penalty", make=make_penalty, call=call_penalty, exact=("value", "g_im", "g_ds"), sync_free=True),
            sc.Case(name="outside_mask", make=make_outside, call=call_outside, exact=("outside", "status"), sync_free=True)]


@pytest.mark.parametrize("case", _stream_cases(), ids=lambda c: c.name)
def test_stream_order(gpu, case):
    """behind a blocker on a fresh stream the buffers are overwritten with the real inputs, the call is made and its outputs cloned
    on that stream, and only the stream is waited for (tests/stream_cases.py): a launch or memset on another stream reads the decoy"""
    sc.run_case(case, gpu)
    print(f"[{case.name}] enqueue {sc.ENQUEUE_MS[case.name]:.3f} ms")


# ---- 3. host synchronisation ------------------------------------------------------------------------------------------------------------

def test_no_host_synchronisation_in_the_mask_and_the_penalty(gpu):
    from fisher_rast import object_loss as ol
    shape = (37, 53)
    ds, gt = (_dev(a, gpu) for a in oc.make_mask_case(shape, "half"))
    im = _dev(oc.make_penalty_case(shape, "plain", "half")[0], gpu).requires_grad_(True)
    dsg = ds.clone().requires_grad_(True)
    obj = _dev(oc.make_obj(shape, "half"), gpu).bool()
    w = torch.tensor(0.5, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for reject, presence in oc.FLAGS:
            for o in (None, obj, obj.view(torch.uint8), obj.float(), obj.unsqueeze(-1)):
                depth, mask = ol.loss_pixel_mask(dsg, gt, oc.SIL_THRES, reject, presence, o)
        (ol.background_penalty(im, dsg, obj) * w).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert mask.dtype == torch.bool and mask.shape == (1,) + shape and depth.data_ptr() == dsg.data_ptr() and depth.shape == (1,) + shape
    assert float(im.grad.abs().sum()) > 0 and float(dsg.grad[1].abs().sum()) > 0 and not bool(dsg.grad[0].any()) and not bool(dsg.grad[2].any())


def test_object_mask_layouts_give_the_same_mask(gpu, h):
    from fisher_rast import object_loss as ol
    shape = (37, 53)
    ds, gt = oc.make_mask_case(shape, "half")
    obj = oc.make_obj(shape, "half")
    want, _ = oc.harness_mask(h, ds, gt, oc.SIL_THRES, True, True, obj)
    dst, gtt = _dev(ds, gpu), _dev(gt, gpu)
    for form in oc.OBJ_FORMS:
        for where in ("cpu", gpu):
            _, mask = ol.loss_pixel_mask(dst, gtt, oc.SIL_THRES, True, True, oc.obj_form(obj, form).to(where))
            assert np.array_equal(mask[0].cpu().numpy(), want.astype(bool)), (form, where)
    b = _dev(obj, gpu).bool()
    assert ol.mask_bytes(b, shape[0], shape[1], b.device).data_ptr() == b.data_ptr()


def _sync_warnings(fn):
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    return out, [w for w in caught if "synchroniz" in str(w.message)]


@pytest.mark.parametrize("i", range(len(oc.GOLDEN_OUTSIDE_CASES)))
def test_get_gaussians_outside_mask_reads_the_host_once_and_gives_the_reference(gpu, golden, i):
    from models.SLAM.utils import slam_external as se
    case = oc.make_golden_outside_case(i)
    params = {k: v.to(gpu) for k, v in oc.trajectory_params(case, t=oc.GOLDEN_FRAME).items()}
    curr = dict(id=oc.GOLDEN_FRAME, intrinsics=_dev(case["K"], gpu))
    obj = _dev(case["obj"], gpu).bool()
    se.get_gaussians_outside_mask(params, curr, obj)                                   # (first use: the library loads)
    (outside, lean), syncs = _sync_warnings(lambda: se.get_gaussians_outside_mask(params, curr, obj, with_indices=False))
    assert len(syncs) == 1, [str(w.message) for w in syncs]
    (outside_i, stats), syncs_i = _sync_warnings(lambda: se.get_gaussians_outside_mask(params, curr, obj))
    print(f"host reads: {len(syncs)} without the index lists, {len(syncs_i)} with them")
    assert hasattr(torch, "nonzero_static") and len(syncs_i) == 1
    assert torch.equal(outside, outside_i) and {k: v for k, v in stats.items() if not k.startswith("idx")} == lean
    assert torch.equal(stats['idx_out'], torch.nonzero(outside).squeeze(1)) and torch.equal(stats['idx_in'], torch.nonzero(~outside).squeeze(1))
    # against the reference's run, outside the band around the decisions (tests/test_object_loss_cpu.py)
    ref64 = dict(case, w2c=np.eye(4))
    ref64["w2c"][:3, :3] = oc.rotation_of(case["quat"].astype(np.float64))
    ref64["w2c"][:3, 3] = case["w2c"][:3, 3]
    want = oc.outside_torch(ref64, torch.float64)
    H, W = case["obj"].shape
    band = oc.outside_band(want["u"], want["v"], want["z"], W, H)
    gold = golden[f"outside/{i}/outside"]
    got = outside.cpu().numpy()
    assert int(band.sum()) <= -(-len(band) // 100) and np.array_equal(got[~band], gold[~band])
    assert stats['total'] == len(gold) and stats['in_count'] == int((~got).sum()) and stats['out_count'] == int(got.sum())
    if np.array_equal(got, gold):
        assert np.allclose([stats[k] for k in ('inside_scale_min', 'inside_scale_max', 'outside_scale_min', 'outside_scale_max')],
                           golden[f"outside/{i}/ranges"], rtol=2e-7, atol=0)


# ---- 4. inside get_loss -------------------------------------------------------------------------------------------------------------------

class _Scene:
    """the 64 x 64, P = 2000 scene of tests/test_gpu_rendervar.py (test_get_loss_with_the_flag_on_against_off) with an object mask"""

    def __init__(self, gpu):
        import rendervar_cases as rc
        from fisher_rast import synthetic
        from models.SLAM.utils.recon_helpers import setup_camera
        from test_gpu_rendervar import _quaternion_of
        self.P, W, H, self.t = 2000, 64, 64, 1
        self.gpu, self.rc = gpu, rc
        self.base = {k: v.contiguous() for k, v in synthetic.room_shell(self.P, seed=12).items()}
        pose = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=13))[0].double().numpy()
        rots = np.tile(np.array([1.0, 0, 0, 0])[None, :, None], (1, 1, 3))
        rots[0, :, self.t] = 1.7 * _quaternion_of(pose[:3, :3])
        trans = np.zeros((1, 3, 3))
        trans[0, :, self.t] = pose[:3, 3]
        self.base["cam_unnorm_rots"], self.base["cam_trans"] = torch.from_numpy(rots).float(), torch.from_numpy(trans).float()
        cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
        first = rc.random_rigid(np.random.default_rng(5))
        first[:3, :3] = 0.9 * np.eye(3) + 0.1 * first[:3, :3]
        g = torch.Generator().manual_seed(3)
        obj = torch.zeros((H, W), dtype=torch.bool)
        obj[8:52, 12:44] = True                                                     # about half of the image
        self.obj = obj.to(gpu)
        self.curr = dict(cam=cam, w2c=torch.from_numpy(first).float().to(gpu), im=torch.rand((3, H, W), generator=g).to(gpu),
                         depth=(torch.rand((1, H, W), generator=g) * 4 + 0.5).to(gpu), obj_mask_2d=self.obj)
        self.curr['depth'][0, :4, :] = 0.0
        self.curr['depth'][0, 20:24, 20:40] = 60.0                                  # far off what the map renders: outliers, inside the object
        self.weights = dict(im=0.5, depth=1.0)

    def transform_to_frame(self, params, time_idx, gaussians_grad, camera_grad):
        rc = self.rc
        cq, ct = params['cam_unnorm_rots'][..., time_idx], params['cam_trans'][..., time_idx]
        if not camera_grad:
            cq, ct = cq.detach(), ct.detach()
        return rc.t_points(rc.t_pose(cq, ct), params['means3D'] if gaussians_grad else params['means3D'].detach())

    def run(self, monkeypatch, tracking, ignore, curr=None, **flags):
        """one get_loss + backward; dict(loss, weighted, mask, im, depth_sil and their gradients, the parameters' gradients)"""
        import models.SLAM.gaussian as G
        from models.SLAM.utils import slam_helpers as sh
        seen = {}
        plain = sh.render_rgb_depth_sil

        def keeping(*a, **k):
            im, radius, depth_sil, rendervar = plain(*a, **k)
            im.retain_grad()
            depth_sil.retain_grad()
            seen.update(im=im, depth_sil=depth_sil)
            return im, radius, depth_sil, rendervar

        inner = sh.calc_loss if tracking else sh.calc_loss_mask

        def calc(curr_data, im, depth, mask, color_mask, *f):
            seen["mask"] = mask.detach().clone()
            return inner(curr_data, im, depth, mask, color_mask, *f)

        monkeypatch.setattr(G, "render_rgb_depth_sil", keeping)
        params = {k: v.clone().to(self.gpu).requires_grad_(True) for k, v in self.base.items()}
        variables = dict(max_2D_radius=torch.zeros(self.P, device=self.gpu), means2D_gradient_accum=torch.zeros(self.P, device=self.gpu),
                         denom=torch.zeros(self.P, device=self.gpu))
        loss, variables, weighted = G.make_get_loss(self.transform_to_frame, calc, **flags)(
            params, self.curr if curr is None else curr, variables, self.t, self.weights, True, 0.5, True, ignore, tracking=tracking, mapping=not tracking)
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        return dict(loss=loss.detach(), weighted={k: v.detach() for k, v in weighted.items()}, mask=seen["mask"], im=seen["im"].detach(),
                    depth_sil=seen["depth_sil"].detach(), d_im=seen["im"].grad, d_depth_sil=seen["depth_sil"].grad,
                    grads={k: None if v.grad is None else v.grad.cpu().numpy() for k, v in params.items()})


@pytest.fixture(scope="module")
def scene(gpu):
    return _Scene(gpu)


@pytest.mark.parametrize("ignore", [False, True], ids=["all-depths", "outliers-rejected"])
@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_get_loss_fused_against_the_torch_route(gpu, scene, monkeypatch, mode, ignore):
    """make_get_loss(object_mask=True, fused_mask=True) against fused_mask=False through the drop-in rasteriser.  Identical masks; the
    depth term, which depends on the mask alone, bit for bit; the loss by the rule, the binary64 evaluation being the torch route's
    loss with its penalty taken in binary64 on the same render (the penalty is all that differs); the gradients w.r.t. the render
    by the rule as well, and the parameters' within the bounds of test_drop_in_get_loss_against_the_two_render_route."""
    import models.SLAM.gaussian as G
    tracking = mode == "tracking"
    fused = scene.run(monkeypatch, tracking, ignore, object_mask=True, fused_mask=True)
    plain = scene.run(monkeypatch, tracking, ignore, object_mask=True, fused_mask=False)
    assert torch.equal(fused["im"], plain["im"]) and torch.equal(fused["depth_sil"], plain["depth_sil"])
    assert torch.equal(fused["mask"], plain["mask"]) and 0 < int(fused["mask"].sum()) <= int(scene.obj.sum())
    assert torch.equal(fused["weighted"]["depth"], plain["weighted"]["depth"])
    w = scene.weights["im"]
    p32 = float(G._background_penalty_torch(plain["im"], plain["depth_sil"][1], scene.obj))
    p64 = float(G._background_penalty_torch(plain["im"].double(), plain["depth_sil"][1].double(), scene.obj))
    loss32 = float(plain["loss"])
    loss64 = loss32 - w * p32 + w * p64
    need = oc.value_need(float(fused["loss"]), loss32, loss64)
    if ignore:
        assert not bool(fused["mask"][0, 20:24, 20:40].any())
    print(f"{mode} ignore={ignore}: loss fused {float(fused['loss'])!r} torch {loss32!r}, need (deviation / bound) {need:.3f}; penalty {p32!r}")
    assert need <= 1.0 and p32 > 0
    # gradients w.r.t. the render: the loss terms' are the same kernels on the same mask, the penalty's are autograd's own values
    for name in ("d_im", "d_depth_sil"):
        a, b = fused[name].cpu().numpy(), plain[name].cpu().numpy()
        assert np.array_equal(a == 0, b == 0), name
        assert oc.grad_need(a, b, b.astype(np.float64)) <= 1.0, name
    wanted = ("cam_unnorm_rots", "cam_trans") if tracking else ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales")
    for k in wanted:
        assert fused["grads"][k] is not None and float(np.abs(plain["grads"][k]).max()) > 0, k
        assert_close(fused["grads"][k], plain["grads"][k], 2e-4, f"get_loss d/d{k}, fused_mask on against off", atol_frac=2e-6)


@pytest.mark.parametrize("mode", ["tracking", "mapping"])
def test_get_loss_with_the_flags_off_is_todays_route(gpu, scene, monkeypatch, mode):
    """With the flags off -- left out, or passed as False -- the step is the parent commit's: the loss, the mask and the gradients
    w.r.t. the render bit for bit, with and without an `obj_mask_2d` in the frame (it is not read).  `fused_mask=True` alone puts the
    same mask on the kernels: again the same bits.  The parameters' gradients come out of the rasteriser's backward, whose float
    atomics do not repeat their own bits from call to call, so they are held to that route's tolerance."""
    tracking = mode == "tracking"
    today = scene.run(monkeypatch, tracking, True)
    no_obj = {k: v for k, v in scene.curr.items() if k != "obj_mask_2d"}
    for curr, flags in ((None, dict(fused_mask=False, object_mask=False)), (no_obj, dict()), (None, dict(fused_mask=True)), (no_obj, dict(fused_mask=True, object_mask=True))):
        got = scene.run(monkeypatch, tracking, True, curr=curr, **flags)
        for k in ("loss", "mask", "im", "depth_sil", "d_im", "d_depth_sil"):
            assert oc.same_bits(got[k].cpu().numpy(), today[k].cpu().numpy()), (flags, k)
        for k, g in today["grads"].items():
            assert (g is None) == (got["grads"][k] is None), k
            if g is not None:
                assert_close(got["grads"][k], g, 2e-4, f"get_loss d/d{k}, flags {flags}", atol_frac=2e-6)


def test_the_object_mask_changes_the_step_as_the_reference_does(gpu, scene, monkeypatch):
    """object_mask=True against False with a half mask: another loss; outside the object mask the render's colour gradient is the
    penalty's and nothing else (the masked L1 sum does not reach there), inside it the penalty adds nothing."""
    from fisher_rast import object_loss as ol
    for fused in (True, False):
        on = scene.run(monkeypatch, True, False, object_mask=True, fused_mask=fused)
        off = scene.run(monkeypatch, True, False, object_mask=False, fused_mask=fused)
        assert float(on["loss"]) != float(off["loss"]) and not torch.equal(on["mask"], off["mask"])
        assert torch.equal(on["mask"], off["mask"] & scene.obj.unsqueeze(0))
        im = on["im"].clone().requires_grad_(True)
        ds = on["depth_sil"].clone().requires_grad_(True)
        (ol.background_penalty(im, ds, scene.obj) * scene.weights["im"]).backward()
        bg = ~scene.obj
        assert float(on["d_im"][:, bg].abs().sum()) > 0
        if fused:
            assert torch.equal(on["d_im"][:, bg], im.grad[:, bg])
        else:
            assert_close(on["d_im"][:, bg].cpu().numpy(), im.grad[:, bg].cpu().numpy(), 1e-6, "penalty gradient outside the mask", atol_frac=0)
        assert not bool(im.grad[:, scene.obj].any()) and not bool(ds.grad[1][scene.obj].any())
        assert torch.equal(on["d_im"][:, scene.obj], off["d_im"][:, scene.obj])


@pytest.mark.parametrize("mode", ["tracking", "mapping"])
@pytest.mark.parametrize("i", range(len(oc.GOLDEN_LOSS_CASES)))
def test_fused_get_loss_reproduces_the_reference(gpu, monkeypatch, golden, i, mode):
    """The fused route of make_get_loss(object_mask=True, fused_mask=True) on the reference's own frames (the render stands in, as in
    the golden script): the mask and the gradients' zero pattern exactly; the depth term exactly where its sum is exact in any order
    (the plateau case: multiples of 1/8), by the rule elsewhere; the values and the gradients by the rule."""
    import models.SLAM.gaussian as G
    from models.SLAM.utils import slam_helpers as sh
    case, run = oc.make_golden_loss_case(i), f"loss/{i}/{mode}"
    im, ds = _dev(case["im"], gpu).requires_grad_(True), _dev(case["depth_sil"], gpu).requires_grad_(True)
    seen = {}
    monkeypatch.setattr(G, "render_rgb_depth_sil", lambda params, cam, w2c, pts, **k: (im, torch.arange(7, device=gpu, dtype=torch.int32) % 3, ds,
                                                                                      dict(means2D=torch.zeros(7, 3, device=gpu))))
    inner = sh.calc_loss if mode == "tracking" else sh.calc_loss_mask

    def calc(curr, im_, depth_, mask, color_mask, *f):
        seen["mask"] = mask.detach().clone()
        return inner(curr, im_, depth_, mask, color_mask, *f)

    ran = []
    from fisher_rast import object_loss as ol
    real = ol.loss_mask_raw
    monkeypatch.setattr(ol, "loss_mask_raw", lambda *a, **k: ran.append(1) or real(*a, **k))
    curr = dict(cam=None, w2c=torch.eye(4, device=gpu), im=_dev(case["gt_im"], gpu), depth=_dev(case["gt"], gpu), obj_mask_2d=_dev(case["obj"], gpu).bool())
    variables = dict(max_2D_radius=torch.zeros(7, device=gpu))
    loss, _, weighted = G.make_get_loss(lambda *a, **k: None, calc, fused_mask=True, object_mask=True)(
        {}, curr, variables, 0, oc.GOLDEN_WEIGHTS, True, oc.SIL_THRES, True, case["ignore"], tracking=mode == "tracking", mapping=mode == "mapping")
    loss.backward()
    torch.cuda.synchronize()
    assert ran, "the fused route was not taken"
    assert np.array_equal(seen["mask"][0].cpu().numpy(), golden[f"{run}/mask"])
    got = np.array([float(weighted[k].detach()) for k in ("im", "depth", "loss")], np.float32)
    if oc.GOLDEN_LOSS_CASES[i][0] == "plateau" and mode == "tracking":
        assert got[1] == golden[f"{run}/weighted"][1]
    for k in range(3):
        need = oc.value_need(got[k], golden[f"{run}/weighted"][k], golden[f"{run}/weighted64"][k])
        assert need <= 1.0, (k, got, golden[f"{run}/weighted"], golden[f"{run}/weighted64"])
    for name, g in (("d_im", im.grad), ("d_depth_sil", ds.grad)):
        a = g.cpu().numpy()
        assert np.array_equal(a == 0, golden[f"{run}/{name}"] == 0), name
        assert oc.grad_need(a, golden[f"{run}/{name}"], golden[f"{run}/{name}64"]) <= 1.0, name
