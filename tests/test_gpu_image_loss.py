"""-m gpu: the fused image loss (fr_image_loss_forward / fr_image_loss_backward, csrc/fr_loss.hip) and what is written on it
(calc_loss / calc_loss_mask / l1_loss_v1 of models/SLAM/utils/slam_helpers.py, calc_ssim / calc_ssim_masked of slam_external.py).

Bit for bit against the g++ harness over the same header (tests/harness/fr_loss_harness.cpp) for every template instance, mask
layout and shape; against the reference's own binary32 / binary64 runs (tests/golden/reference_loss.npz) by the rule of
tests/test_image_loss_cpu.py; no host synchronisation on the way; and inside `make_get_loss` against the torch chain written out
here."""
import ctypes

import numpy as np
import pytest
import torch

import loss_cases as lc
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

GUARD = 64                    # floats behind every output
GUARD_BITS = 0x5A5A5A5A
UPSTREAM = 0.37               # not 1: the kernel has to read it
SHAPES = lc.SHAPES + [(1, 1, 1), (3, 16, 16), (3, 37, 53), (3, 256, 256)]


@pytest.fixture(scope="module")
def loss_harness():
    return lc.build_harness()


@pytest.fixture(scope="module")
def fixture():
    return lc.load_fixture()


def _instances(C):
    """One term per template instance <SSIM, MASKED>, both mask layouts, and the weighted-map role"""
    out = [lc.Term("ssim+l1", 0.8, 0.2, lc.L1_MEAN), lc.Term("l1", 1.0, 0.0, lc.L1_SUM),
           lc.Term("ssim+l1 masked [C]", 0.8, 0.2, lc.L1_MASKED_MEAN, "c"), lc.Term("l1 masked [C]", 1.0, 0.0, lc.L1_SUM, "c"),
           lc.Term("l1 masked mean [1]", 1.0, 0.0, lc.L1_MASKED_MEAN, "1"), lc.Term("ssim+l1 masked [1]", 0.8, 0.2, lc.L1_MASKED_MEAN, "1"),
           lc.Term("ssim weighted [1]", 0.0, -1.0, lc.L1_SUM, "1", True, "ssim")]
    return out


class _Guarded:
    """a device buffer of n elements with GUARD words behind it"""

    def __init__(self, n, dev, dtype=torch.float32):
        words = n * (2 if dtype == torch.float64 else 1)
        self.buf = torch.full((words + GUARD,), GUARD_BITS, dtype=torch.int32, device=dev)
        self.n, self.words, self.dtype = n, words, dtype

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self):
        return self.buf[:self.words].view(self.dtype).cpu().numpy()

    def intact(self):
        return bool((self.buf[self.words:] == GUARD_BITS).all())


def _abi(dev, x, y, mask, term, upstream=UPSTREAM):
    """forward + backward through the C ABI on guarded buffers; returns the outputs as NumPy and whether every guard is intact"""
    from fisher_rast import _lib
    lib = _lib.load()
    C, H, W = x.shape
    n = C * H * W
    ssim = term.w_ssim != 0.0
    xt, yt = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)
    mt = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).to(dev)
    cfg = _lib.ImageLossCfg(C, H, W, term.w_l1, term.w_ssim, term.denom, 0 if mask is None else (1 if mask.shape[0] == 1 and C != 1 else C),
                            int(term.weights_map))
    nws = int(lib.fr_image_loss_workspace_bytes(C, H, W))
    assert nws % 8 == 0 and nws >= 3 * C * ((H + 15) // 16) * ((W + 15) // 16) * 8
    out4, chan, smap = _Guarded(4, dev), _Guarded(C, dev), _Guarded(n, dev)
    saved, ws, grad = _Guarded((3 * n if ssim else 0) + 4, dev), _Guarded(nws // 8, dev, torch.float64), _Guarded(n, dev)
    up = torch.tensor([upstream], dtype=torch.float32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _lib.check(lib.fr_image_loss_forward(ctypes.byref(cfg), xt.data_ptr(), yt.data_ptr(), None if mt is None else mt.data_ptr(), out4.ptr,
                                         chan.ptr if ssim else None, smap.ptr if ssim else None, saved.ptr, ws.ptr, nws, stream),
               "fr_image_loss_forward")
    _lib.check(lib.fr_image_loss_backward(ctypes.byref(cfg), xt.data_ptr(), yt.data_ptr(), None if mt is None else mt.data_ptr(), saved.ptr,
                                          up.data_ptr(), grad.ptr, stream), "fr_image_loss_backward")
    torch.cuda.synchronize()
    res = dict(out=out4.get(), saved=saved.get(), grad=grad.get().reshape(C, H, W))
    if ssim:
        res.update(channel_ssim=chan.get(), ssim_map=smap.get().reshape(C, H, W))
    return res, all(g.intact() for g in (out4, chan, smap, saved, ws, grad))


def _same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def _within_one_ulp(got32, want64):
    if np.isnan(want64):
        return bool(np.isnan(got32))
    return abs(float(got32) - float(want64)) <= float(np.spacing(np.float32(abs(want64))))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_are_the_harness_bit_for_bit(gpu, loss_harness, shape):
    """ssim map, saved partials and dL_dimg as uint32; the loss within 1 binary32 ulp of the harness's fp64 sum; a second call gives
    the same bits; the guard words stay"""
    families = lc.FAMILIES if shape in lc.SHAPES else ["noise"]
    kinds = ["half", "empty"] if shape in lc.SHAPES else ["half"]
    for family in families:
        for kind in kinds:
            x, y, m1, mc = lc.make_case(shape, family, kind)
            for term in _instances(shape[0]):
                if kind == "empty" and term.mask == "none":
                    continue
                mask = term.pick_mask(m1, mc)
                want = lc.harness_forward(loss_harness, x, y, mask, term.w_l1, term.w_ssim, term.denom, term.weights_map)
                want_grad = lc.harness_backward(loss_harness, x, y, mask, term.w_ssim, want["saved"], UPSTREAM, term.weights_map)
                got, intact = _abi(gpu, x, y, mask, term)
                tag = (shape, family, kind, term.name)
                assert intact, tag
                assert _same_bits(got["saved"], want["saved"]), tag
                assert _same_bits(got["grad"], want_grad), tag
                if term.w_ssim != 0.0:
                    assert _same_bits(got["ssim_map"], want["ssim_map"]), tag
                    assert np.allclose(got["channel_ssim"], want["channel_ssim"], rtol=2e-7, atol=0), tag
                for k in range(4):
                    assert _within_one_ulp(got["out"][k], want["out"][k]), (tag, k, got["out"], want["out"])
                if kind == "empty" and term.mask != "none" and not term.weights_map:
                    assert not got["grad"].any(), tag
                if family == families[0]:
                    again, _ = _abi(gpu, x, y, mask, term)
                    assert all(np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)) for k in got), tag


def _product_term(name, xt, yt, m1t, mct):
    """the product's function for a fixture term (what make_reference_loss_vectors.py asked of the reference's)"""
    from models.SLAM.utils import slam_external as se, slam_helpers as sh
    C, H, W = xt.shape
    d3, d1 = torch.zeros((3, H, W), device=xt.device), torch.zeros((1, H, W), device=xt.device)
    if name == "ssim":
        return se.calc_ssim(xt, yt)
    if name == "ssim_masked":
        return se.calc_ssim_masked(xt, yt, m1t)
    if name == "map_im":
        return sh.calc_loss(dict(im=yt, depth=d1), xt, d1, m1t, mct, False, False, False, False)["im"]
    if name == "trk_im":
        return sh.calc_loss(dict(im=yt, depth=d1), xt, d1, m1t, mct, False, False, False, True)["im"]
    if name == "trk_im_masked":
        return sh.calc_loss(dict(im=yt, depth=d1), xt, d1, m1t, mct, False, True, False, True)["im"]
    if name == "mapmask_im":
        return sh.calc_loss_mask(dict(im=yt, depth=d1), xt, d1, m1t, mct, False, False, False, False)["im"]
    if name == "map_depth":
        return sh.calc_loss(dict(im=d3, depth=yt), d3, xt, m1t, m1t.repeat(3, 1, 1), True, False, False, False)["depth"]
    if name == "trk_depth":
        return sh.calc_loss(dict(im=d3, depth=yt), d3, xt, m1t, m1t.repeat(3, 1, 1), True, False, False, True)["depth"]
    raise ValueError(name)


@pytest.mark.parametrize("family", lc.FAMILIES)
@pytest.mark.parametrize("shape", lc.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_product_functions_against_the_reference_by_the_rule(gpu, fixture, shape, family):
    """calc_ssim / calc_ssim_masked / calc_loss / calc_loss_mask of the package, value and autograd gradient, against what the
    reference's functions gave on the CPU, by the rule of test_image_loss_cpu.py; prints the need (deviation / bound)."""
    n = shape[0] * shape[1] * shape[2]
    need, failures = np.zeros(2), []
    for kind in lc.MASK_KINDS:
        x, y, m1, mc = lc.make_case(shape, family, kind)
        yt, m1t, mct = torch.from_numpy(y).to(gpu), torch.from_numpy(m1).to(gpu), torch.from_numpy(mc).to(gpu)
        for term in lc.terms_for(shape[0], kind):
            v32, v64, gdev, g64 = fixture[0][lc.key(shape, family, kind, term.name)]
            if not g64.size:
                g64 = lc.loss64(x, y, term.pick_mask(m1, mc), term.w_l1, term.w_ssim, term.denom, term.weights_map)[1].reshape(-1)
            xt = torch.from_numpy(x).to(gpu).requires_grad_(True)
            v = _product_term(term.name, xt, yt, m1t, mct)
            v.backward()
            grad = xt.grad.cpu().numpy()
            assert not np.isnan(grad).any(), (kind, term.name)
            lneed, gneed = lc.needs(term, n, float(v.detach()), grad, v32, v64, g64, gdev)
            need = np.maximum(need, [lneed, gneed])
            if lneed > 1.0 or gneed > 1.0:
                failures.append((kind, term.name, lneed, gneed))
    print(f"GPU need (deviation / bound) {shape} {family:9s}: loss {need[0]:.3f}  gradient {need[1]:.3f}")
    assert not failures, failures


def test_batch_folds_into_channels_and_autograd_equals_the_abi(gpu, loss_harness):
    from models.SLAM.utils import slam_external as se, slam_helpers as sh
    x0, y0, _, _ = lc.make_case((3, 17, 33), "noise", "none")
    x1, y1, m1, mc = lc.make_case((3, 17, 33), "smooth", "half")
    xb, yb = np.stack([x0, x1]), np.stack([y0, y1])                     # [2,3,17,33]
    xt = torch.from_numpy(xb).to(gpu).requires_grad_(True)
    yt = torch.from_numpy(yb).to(gpu)
    (se.calc_ssim(xt, yt) * UPSTREAM).backward()
    folded = torch.from_numpy(xb.reshape(6, 17, 33)).to(gpu).requires_grad_(True)
    vf = se.calc_ssim(folded, yt.reshape(6, 17, 33))
    (vf * UPSTREAM).backward()
    assert torch.equal(se.calc_ssim(xt, yt).detach(), vf.detach()) and torch.equal(xt.grad.reshape(6, 17, 33), folded.grad)
    want = lc.harness_forward(loss_harness, xb.reshape(6, 17, 33), yb.reshape(6, 17, 33), None, 0.0, -1.0, lc.L1_SUM)
    assert _within_one_ulp(float(vf.detach()), want["out"][2])
    per_batch = se.calc_ssim(xt.detach(), yt, size_average=False).cpu().numpy()
    assert per_batch.shape == (2,) and np.allclose(per_batch, want["channel_ssim"].reshape(2, 3).mean(1), rtol=1e-6, atol=0)
    with pytest.raises(NotImplementedError):
        se.calc_ssim(xt, yt, window_size=7)
    with pytest.raises(NotImplementedError):
        se.calc_ssim(xt.detach(), yt.clone().requires_grad_(True))
    # the autograd route of calc_loss / calc_loss_mask / l1_loss_v1 against the direct ABI call with the same upstream gradient
    m1t, mct = torch.from_numpy(m1).to(gpu), torch.from_numpy(mc).to(gpu)
    d1 = torch.zeros((1, 17, 33), device=gpu)
    for fn, term, mask in ((sh.calc_loss, lc.Term("map_im", 0.8, 0.2, lc.L1_MEAN), None),
                           (sh.calc_loss_mask, lc.Term("mapmask_im", 0.8, 0.2, lc.L1_MASKED_MEAN, "c"), mc)):
        xa = torch.from_numpy(x1).to(gpu).requires_grad_(True)
        v = fn(dict(im=torch.from_numpy(y1).to(gpu), depth=d1), xa, d1, m1t, mct, False, False, False, False)["im"]
        (v * UPSTREAM).backward()
        got, intact = _abi(gpu, x1, y1, mask, term)
        assert intact and _same_bits(xa.grad.cpu().numpy(), got["grad"]) and _same_bits(v.detach().cpu().numpy(), got["out"][0])
    xa = torch.from_numpy(x1).to(gpu).requires_grad_(True)
    (sh.l1_loss_v1(xa, torch.from_numpy(y1).to(gpu)) * UPSTREAM).backward()
    got, _ = _abi(gpu, x1, y1, None, lc.Term("l1 mean", 1.0, 0.0, lc.L1_MEAN))
    assert _same_bits(xa.grad.cpu().numpy(), got["grad"])


def test_no_host_synchronisation_on_the_fused_path(gpu):
    """the reference's chain synchronises twice per iteration (boolean indexing); the fused calc_loss / calc_loss_mask must not at all"""
    from models.SLAM.utils import slam_helpers as sh
    x, y, m1, mc = lc.make_case((3, 37, 53), "smooth", "half")
    xd, yd, _, _ = lc.make_case((1, 37, 53), "noise", "half")
    t = lambda a: torch.from_numpy(a).to(gpu)
    im, depth = t(x).requires_grad_(True), t(xd).requires_grad_(True)
    curr = dict(im=t(y), depth=t(yd))
    m1t = t(m1)
    w_im, w_depth = torch.tensor(0.5, device=gpu), torch.tensor(1.0, device=gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for fn in (sh.calc_loss, sh.calc_loss_mask):
            for tracking, sil in ((False, False), (True, True), (True, False)):
                terms = fn(curr, im, depth, m1t, m1t.repeat(3, 1, 1), True, sil, False, tracking)
                (terms['im'] * w_im + terms['depth'] * w_depth).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(im.grad).all()) and bool(torch.isfinite(depth.grad).all()) and float(im.grad.abs().sum()) > 0


def test_get_loss_with_the_fused_loss_against_the_torch_chain(gpu):
    """`make_get_loss` with the package's calc_loss on the scene of test_drop_in_get_loss_against_the_two_render_route, against the
    reference's structure (two renders, the torch chain written out below).  The two loss terms and their gradients w.r.t. the
    rendered images agree by the rule, D_ref being the deviation of the torch chain in binary32 from the same chain in binary64 on
    the same render; then, the rasteriser's backward being linear in the image gradients, the two-render route driven with the FUSED
    image gradients must give the Gaussians' gradients of the fused route within that test's own tolerance."""
    import torch.nn.functional as F
    from diff_gaussian_rasterization import GaussianRasterizer as Renderer
    from fisher_rast import synthetic
    from models.SLAM.gaussian import make_get_loss
    from models.SLAM.utils import slam_helpers as sh
    from models.SLAM.utils.recon_helpers import setup_camera
    P, W, H = 5000, 96, 80
    base = synthetic.room_shell(P, seed=12)
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=13))[0].to(gpu)
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    g = torch.Generator().manual_seed(3)
    curr_data = dict(cam=cam, w2c=torch.eye(4, device=gpu), im=torch.rand((3, H, W), generator=g).to(gpu),
                     depth=(torch.rand((1, H, W), generator=g) * 4 + 0.5).to(gpu))
    curr_data['depth'][0, :4, :] = 0.0

    def transform_to_frame(params, time_idx, gaussians_grad, camera_grad):
        pts = params['means3D'] if gaussians_grad else params['means3D'].detach()
        return (w2c @ torch.cat((pts, torch.ones_like(pts[:, :1])), 1).T).T[:, :3]

    taps = torch.from_numpy(lc.TAPS_BITS.view(np.float32).copy())
    window = (taps[:, None] * taps[None, :]).to(gpu)

    def torch_chain(curr, im, depth, mask, dtype):
        """the parent commit's loss: masked-mean L1 depth, 0.8 mean L1 + 0.2 (1 - ssim) colour, in `dtype`"""
        x, y, w = im.to(dtype), curr['im'].to(dtype), window.to(dtype).expand(3, 1, 11, 11).contiguous()
        blur = lambda a: F.conv2d(a[None], w, padding=5, groups=3)[0]
        mu1, mu2 = blur(x), blur(y)
        s1, s2, s12 = blur(x * x) - mu1 * mu1, blur(y * y) - mu2 * mu2, blur(x * y) - mu1 * mu2
        ssim = ((2 * mu1 * mu2 + 0.01 ** 2) * (2 * s12 + 0.03 ** 2)) / ((mu1 * mu1 + mu2 * mu2 + 0.01 ** 2) * (s1 + s2 + 0.03 ** 2))
        return dict(depth=torch.abs(curr['depth'].to(dtype) - depth.to(dtype))[mask].mean(),
                    im=0.8 * torch.abs(x - y).mean() + 0.2 * (1.0 - ssim.mean()))

    weights = dict(im=0.5, depth=1.0)
    seen = {}

    def fused_calc_loss(curr, im, depth, mask, color_mask, *flags):
        im.retain_grad(); depth.retain_grad()
        seen.update(im=im, depth=depth, mask=mask, terms=sh.calc_loss(curr, im, depth, mask, color_mask, *flags))
        return seen['terms']

    def fresh():
        params = {k: v.clone().to(gpu).requires_grad_(True) for k, v in base.items()}
        variables = dict(max_2D_radius=torch.full((P,), 3.0, device=gpu), means2D_gradient_accum=torch.zeros(P, device=gpu), denom=torch.zeros(P, device=gpu))
        return params, variables

    params, variables = fresh()
    loss, variables, wl = make_get_loss(transform_to_frame, fused_calc_loss)(params, curr_data, variables, 0, weights, True, 0.5, True, False, mapping=True)
    loss.backward()
    # the reference's structure on the same parameters
    params2, _ = fresh()
    tp = transform_to_frame(params2, 0, True, False)
    rv = sh.transformed_params2rendervar(params2, tp)
    ds = sh.transformed_params2depthplussilhouette(params2, curr_data['w2c'], tp)
    im2, radius, _ = Renderer(raster_settings=cam)(**rv)
    depth_sil, _, _ = Renderer(raster_settings=cam)(**ds)
    depth2 = depth_sil[0].unsqueeze(0)
    assert torch.equal(im2, seen['im']) and torch.equal(depth2, seen['depth'])
    mask = seen['mask']
    n_im, n_depth = 3 * H * W, H * W
    for name, term, n in (("im", lc.Term("im", 0.8, 0.2, lc.L1_MEAN), n_im), ("depth", lc.Term("depth", 1.0, 0.0, lc.L1_MASKED_MEAN, "1"), n_depth)):
        res = {}
        for dtype in (torch.float32, torch.float64):
            a, b = im2.detach().to(dtype).requires_grad_(True), depth2.detach().to(dtype).requires_grad_(True)
            v = torch_chain(curr_data, a, b, mask, dtype)[name]
            gr, = torch.autograd.grad(v, a if name == "im" else b)
            res[dtype] = (float(v.detach()), gr.double().cpu().numpy())
        (v32, g32), (v64, g64) = res[torch.float32], res[torch.float64]
        got_g = seen[name].grad.cpu().numpy().astype(np.float64) / weights[name]        # 0.5 and 1.0: exact
        lneed, gneed = lc.needs(term, n, float(seen['terms'][name].detach()), got_g, v32, v64, g64, np.abs(g32 - g64).max())
        print(f"get_loss term {name}: need (deviation / bound) loss {lneed:.3f}  gradient {gneed:.3f}")
        assert lneed <= 1.0 and gneed <= 1.0, (name, lneed, gneed)
    torch.autograd.backward([im2, depth2], [seen['im'].grad, seen['depth'].grad])
    for k in ('means3D', 'rgb_colors', 'unnorm_rotations', 'logit_opacities', 'log_scales'):
        assert_close(params[k].grad.cpu().numpy(), params2[k].grad.cpu().numpy(), 2e-4, f"fused-loss get_loss d/d{k}", atol_frac=2e-6)
    assert float(params['means3D'].grad.abs().sum()) > 0 and torch.equal(variables['seen'], radius > 0)
