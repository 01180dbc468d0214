"""-m gpu: the render-quality evaluation (fr_view_metrics / ops.view_metrics / GaussianSLAM.eval_views) against the g++ harness over
the same arithmetic, against the image-loss kernel, and end to end against the per-pose route on a synthetic scene."""
import numpy as np
import pytest
import torch

import eval_cases as ec
import loss_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eval_harness():
    return ec.build_harness()


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _dev(a, gpu):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _run(b, layout, gpu, clamp=True, valid_only=False, depth=True):
    from fisher_rast import ops
    r = ops.view_metrics(_dev(b["render"], gpu), _dev(ec.target_of(b, layout), gpu), _dev(b["depth"], gpu) if depth else None,
                         _dev(b["gt_depth"], gpu) if depth else None, _dev(b["mask"], gpu), clamp=clamp, depth_valid_only=valid_only)
    return r["rows"], r["summary"]


# ---- 1. kernel against harness --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ec.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_against_harness_on_every_case(gpu, eval_harness, shape):
    """every row entry within 1 ulp of binary32 of the harness (the order of the binary64 sums is the one freedom), infinities and
    NaNs in the same places, the summary that of the kernel's own rows bit for bit, and two calls the same bits"""
    worst, n = 0.0, 0
    for s, rot, kind, clamp in ec.all_cases():
        if s != shape:
            continue
        b = ec.make_batch(s, rot, kind)
        for valid_only in (False, True):
            want, _ = ec.harness_metrics(eval_harness, b["render"], b["gt_f32"], b["depth"], b["gt_depth"], b["mask"], clamp, valid_only)
            for layout in ec.LAYOUTS:
                rows, summary = _run(b, layout, gpu, clamp, valid_only)
                again, summary2 = _run(b, layout, gpu, clamp, valid_only)
                got = rows.cpu().numpy()
                d = ec.ulp_diff(got, want)
                worst, n = max(worst, float(d.max())), n + 1
                assert d.max() <= 1, (ec.key(s, rot, kind, clamp), layout, valid_only, got, want)
                assert np.array_equal(bits(rows), bits(again)) and np.array_equal(bits(summary), bits(summary2))
                assert np.array_equal(bits(summary), ec.harness_summary(eval_harness, got).view(np.uint32))
    print(f"{shape}: {n} calls, worst {worst:.0f} ulp")


def test_colour_only_and_out_tensors(gpu, eval_harness):
    from fisher_rast import ops
    b = ec.make_batch((5, 17, 33), 1, "half")
    rows, summary = _run(b, "u8x4", gpu, depth=False)
    want, want_s = ec.harness_metrics(eval_harness, b["render"], b["gt_u8x4"], None, None, b["mask"])
    assert ec.ulp_diff(rows.cpu().numpy(), want).max() <= 1 and torch.isnan(rows[:, [2, 3, 7]]).all()
    out = {"rows": torch.full((5, 8), 7.0, device=gpu), "summary": torch.full((8,), 7.0, device=gpu)}
    r = ops.view_metrics(_dev(b["render"], gpu), _dev(b["gt_u8x4"], gpu), mask=_dev(b["mask"], gpu).bool(), out=out)
    assert r["rows"] is out["rows"] and np.array_equal(bits(out["rows"]), bits(rows)) and np.array_equal(bits(out["summary"]), bits(summary))
    assert np.array_equal(bits(ops.view_metrics_summary(rows)), bits(summary))
    x, g = _dev(b["render"], gpu), _dev(b["gt_f32"], gpu)
    for bad in (dict(render=x.double()), dict(gt_rgb=g.double()), dict(gt_rgb=g.cpu()), dict(gt_rgb=g[:, :, :, :-1]), dict(depth=x[:, 0]),
                dict(depth=x[:, 0].transpose(1, 2).contiguous().transpose(1, 2), gt_depth=x[:, 0]), dict(depth=x[:, 0].half(), gt_depth=x[:, 0]),
                dict(render=x[:, :, :, ::2]), dict(mask=torch.ones((5, 17, 33), device=gpu))):
        with pytest.raises(ValueError):
            ops.view_metrics(**{**dict(render=x, gt_rgb=g), **bad})


# ---- 2. batch identity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ec.LAYOUTS)
def test_a_batch_is_its_views_one_by_one(gpu, layout):
    b = ec.make_batch((5, 17, 33), 3, "half")
    for valid_only in (False, True):
        rows, _ = _run(b, layout, gpu, valid_only=valid_only)
        for v in range(5):
            one = {k: (a[v:v + 1] if isinstance(a, np.ndarray) else a) for k, a in b.items()}
            row, summary = _run(one, layout, gpu, valid_only=valid_only)
            assert np.array_equal(bits(row[0]), bits(rows[v])), (v, b["families"][v])
            assert float(summary[7]) == 1.0


# ---- 3. a strided depth ---------------------------------------------------------------------------------------------------------
def test_depth_as_a_channel_slice_is_taken_where_it_lies(gpu):
    from fisher_rast import ops
    b = ec.make_batch((5, 17, 33), 0, "none")
    depth = _dev(b["depth"], gpu)
    packed = torch.full((5, 3, 17, 33), 1e9, device=gpu)
    packed[:, 0] = depth
    x, g, gd = _dev(b["render"], gpu), _dev(b["gt_u8"], gpu), _dev(b["gt_depth"], gpu)
    a = ops.view_metrics(x, g, packed[:, 0:1], gd.unsqueeze(1))
    c = ops.view_metrics(x, g, depth, gd)
    assert not packed[:, 0:1].is_contiguous() and packed[:, 0:1].data_ptr() == packed.data_ptr()
    assert np.array_equal(bits(a["rows"]), bits(c["rows"])) and np.array_equal(bits(a["summary"]), bits(c["summary"]))
    # and a render whose views are strided (every other view of a larger batch)
    big = torch.zeros((10, 3, 17, 33), device=gpu)
    big[::2] = x
    s = ops.view_metrics(big[::2], g, depth, gd)
    assert np.array_equal(bits(s["rows"]), bits(c["rows"]))


# ---- 4. against the image-loss kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot", [0, 5])
def test_ssim_is_the_image_loss_kernels(gpu, rot):
    """one view, float target, no clamp, no mask: within 2 ulp of fr_image_loss_forward's SSIM mean (out4[2], w_ssim = 1, w_l1 = 0).
    Every view of the two batches but the black target: there every window mean of the target is below 2^-5, the evaluation takes
    the raw moments (fr_eval_math.h: fre_window_is_dark) and the image loss, whose moments about 0.5 miss the reference by 19
    times the rule's bound on such a target, is no yardstick -- that view is held to the reference's own run instead."""
    from fisher_rast import image_loss as il
    from fisher_rast import ops
    b = ec.make_batch((5, 17, 33), rot, "none")
    ref = ec.load_fixture().get(ec.key((5, 17, 33), rot, "none", False))
    checked = 0
    for v in range(5):
        x, y = _dev(b["render"][v], gpu), _dev(b["gt_f32"][v], gpu)
        out4 = il.forward_raw(x, y, None, 0.0, 1.0, il.FR_LOSS_L1_SUM)[0]
        row = ops.view_metrics(x[None], y[None], clamp=False)["rows"][0]
        if b["families"][v] == "black_gt":
            assert ec.need(float(row[1]), ref[v, 0, 1], ref[v, 1, 1]) <= 1.0
            continue
        d = ec.ulp_diff(row[1:2].cpu().numpy(), out4[2:3].cpu().numpy())
        assert d.max() <= 2, (b["families"][v], float(row[1]), float(out4[2]), d)
        checked += 1
    assert checked >= 4


# ---- 5. end to end --------------------------------------------------------------------------------------------------------------
def _ssim64(x, y):
    return float(lc.loss64(x.cpu().numpy(), y.cpu().numpy(), None, 0.0, -1.0, lc.L1_SUM)[0][2])


def test_eval_views_gives_what_the_per_pose_route_gives(gpu):
    """slam.eval_views against render_at_pose, clamp, calc_psnr(...).mean(), mean |depth - depth_gt|, the product's calc_ssim and the
    isinf skip, per pose.  Each value by the rule: within 2 D_ref + 64 2^-24 |value| of that route's expressions in binary64 on
    its own images, D_ref the deviation of its binary32 run."""
    from fisher_rast import synthetic
    from models.SLAM.gaussian import GaussianSLAM
    from models.SLAM.gaussian_object import GaussianObjectSLAM
    from models.SLAM.utils.slam_external import calc_psnr, calc_ssim
    W, H, V = 64, 48, 5
    params = synthetic.room_shell(2000, seed=3)
    slam = GaussianSLAM(params=params, intrinsics=synthetic.intrinsics(W, H), width=W, height=H, device=gpu)
    c2ws = synthetic.candidate_poses(V, seed=5).clone()
    c2ws[3] = torch.eye(4)                  # (its inverse and its camera-frame means are exact on both routes: the same image, bit for bit)
    batch = slam.render_at_poses(c2ws)
    g = torch.Generator().manual_seed(11)
    base = batch["render"].clamp(0.0, 1.0).cpu()
    noisy = (base + 0.1 * torch.randn(base.shape, generator=g)).clamp(0.0, 1.0)
    rgb_gt = torch.round(noisy * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()                    # Habitat's layout, [V,H,W,3]
    rgb_gt = torch.cat((rgb_gt, torch.randint(0, 256, (V, H, W, 1), generator=g, dtype=torch.uint8)), dim=-1)   # ... RGBA
    depth_gt = (batch["depth"].cpu() + 0.05 * torch.randn((V, 1, H, W), generator=g)).clamp_min(0.0)
    gt_f32 = (rgb_gt[..., :3].permute(0, 3, 1, 2) / 255).contiguous().to(gpu)
    gt_f32[3] = batch["render"][3].clamp(0.0, 1.0)          # one pose's target is its own clamped render: PSNR +inf, left out
    rgb_gt, depth_gt = rgb_gt.to(gpu), depth_gt.to(gpu)

    seen = []

    def on_chunk(v0, v1, render, depth):
        assert render.shape == (v1 - v0, 3, H, W) and depth.shape == (v1 - v0, 1, H, W)
        assert float(render.min()) >= 0.0 and float(render.max()) <= 1.0
        assert torch.equal(render, batch["render"][v0:v1].clamp(0.0, 1.0)) and torch.equal(depth, batch["depth"][v0:v1])
        seen.append((v0, v1))
    ev = slam.eval_views(c2ws, gt_f32, depth_gt, chunk=2, on_chunk=on_chunk)
    assert seen == [(0, 2), (2, 4), (4, 5)]
    assert ev.rows.shape == (V, 8) and ev.rows.is_cuda and ev.psnr.shape == (V,) and ev.psnr.dtype == torch.float32 and not ev.psnr.is_cuda

    # the per-pose route
    want32, want64, kept = [], [], []
    for v in range(V):
        pkg = slam.render_at_pose(c2ws[v])
        color = pkg["render"].detach().clone()
        color.clamp_(min=0., max=1.)
        depth = pkg["depth"].detach()
        psnr = calc_psnr(color, gt_f32[v]).mean()
        depth_mae = torch.mean(torch.abs(depth - depth_gt[v]))
        ssim_score = calc_ssim(color.unsqueeze(0), gt_f32[v].unsqueeze(0))
        kept.append(not bool(torch.isinf(psnr)))
        want32.append([float(psnr), float(ssim_score), float(depth_mae)])
        c64, g64 = color.double(), gt_f32[v].double()
        mse64 = ((c64 - g64) ** 2).reshape(3, -1).mean(1)
        want64.append([float((20 * torch.log10(1.0 / torch.sqrt(mse64))).mean()), _ssim64(color, gt_f32[v]),
                       float(torch.mean(torch.abs(depth.double() - depth_gt[v].double())))])
    assert kept == [True, True, True, False, True] and ev.kept.tolist() == kept
    got = torch.stack((ev.psnr, ev.ssim, ev.depth_mae), dim=1).numpy()
    for v in range(V):
        for k, name in enumerate(("psnr", "ssim", "depth_mae")):
            n = ec.need(got[v, k], want32[v][k], want64[v][k])
            print(f"view {v} {name}: eval_views {got[v, k]:.9g}  route32 {want32[v][k]:.9g}  route64 {want64[v][k]:.9g}  need {n:.3g}")
            assert n <= 1.0, (v, name, got[v, k], want32[v][k], want64[v][k], n)
    assert ev.psnr[3] == np.inf and ev.ssim[3] == 1.0
    k = np.array(kept)
    for name, col in (("psnr", 0), ("ssim", 1), ("depth_mae", 2)):
        m32, m64 = float(np.mean(np.array(want32)[k, col])), float(np.mean(np.array(want64)[k, col]))
        assert ec.need(ev.mean[name], m32, m64) <= 1.0, (name, ev.mean[name], m32, m64)
    assert ev.n_kept == 4 and float(ev.summary[7]) == V

    # without a callback (the route with one host read), in another chunking, from bytes on the host: the same rows
    rgba = rgb_gt.clone()
    rgba[3, :, :, :3] = torch.round(gt_f32[3].permute(1, 2, 0) * 255).to(torch.uint8)
    ev_f = slam.eval_views(c2ws, gt_f32, depth_gt, chunk=64)
    assert np.array_equal(bits(ev_f.rows), bits(ev.rows)) and np.array_equal(ev_f.summary.numpy().view(np.uint32), ev.summary.numpy().view(np.uint32))
    ev_b = slam.eval_views(c2ws, rgba.cpu(), depth_gt.cpu(), chunk=3)
    ev_b2 = slam.eval_views(c2ws, (rgba.cpu()[..., :3].permute(0, 3, 1, 2) / 255).contiguous().to(gpu), depth_gt, chunk=2)
    assert np.array_equal(bits(ev_b.rows), bits(ev_b2.rows))
    keep = [0, 1, 2, 4]
    assert np.array_equal(bits(ev_b.rows[keep]), bits(ev.rows[keep]))
    # colour only, and the object class inherits the methods
    ev_c = GaussianObjectSLAM(params=params, intrinsics=synthetic.intrinsics(W, H), width=W, height=H, device=gpu).eval_views(c2ws, gt_f32)
    assert torch.isnan(ev_c.depth_mae).all() and np.isnan(ev_c.mean["depth_mae"]) and torch.equal(ev_c.psnr, ev.psnr) and torch.equal(ev_c.ssim, ev.ssim)


def test_frame_metrics_is_report_progress_for_one_frame(gpu, eval_harness):
    from models.SLAM.gaussian import GaussianSLAM
    b = ec.make_batch((5, 17, 33), 0, "half")
    slam = GaussianSLAM(device=gpu)
    for v in range(3):
        for mask in (None, b["mask"][v]):
            got = slam.frame_metrics(_dev(b["render"][v], gpu), _dev(b["gt_f32"][v], gpu), _dev(b["depth"][v:v + 1], gpu),
                                     _dev(b["gt_depth"][v], gpu), None if mask is None else _dev(mask, gpu).bool())
            want, _ = ec.harness_metrics(eval_harness, b["render"][v:v + 1], b["gt_f32"][v:v + 1], b["depth"][v:v + 1], b["gt_depth"][v:v + 1],
                                         None if mask is None else mask[None], clamp=False, valid_only=True)
            assert ec.ulp_diff(got["row"].cpu().numpy(), want[0]).max() <= 1
            assert got["psnr"].dim() == 0 and float(got["depth_l1"]) == float(got["row"][2])


# ---- 6. stream order ------------------------------------------------------------------------------------------------------------
def test_view_metrics_in_stream_order(gpu):
    """tests/test_gpu_streams.py's procedure (tests/stream_cases.py) for this entry point: behind a blocker on a fresh stream the
    inputs are overwritten, the call is made, the outputs are cloned on the stream: the default-stream bits"""
    import stream_cases as sc

    def make(which):
        b = ec.make_batch((5, 17, 33), (0, 2)[which], "half")
        packed = np.zeros((5, 3, 17, 33), np.float32)
        packed[:, 0] = b["depth"]
        return dict(render=b["render"], gt=b["gt_u8x4"], depth=packed, gt_depth=b["gt_depth"], mask=b["mask"])

    def call(ctx, b):
        from fisher_rast import ops
        r = ops.view_metrics(b["render"], b["gt"], b["depth"][:, 0:1], b["gt_depth"], b["mask"])
        return dict(rows=r["rows"], summary=r["summary"])
    sc.run_case(sc.Case(name="view_metrics", make=make, call=call, exact=("rows", "summary"), sync_free=True), gpu)


# ---- 7. the drop-ins ------------------------------------------------------------------------------------------------------------
def test_calc_psnr_and_calc_mse_drop_ins(gpu):
    from models.SLAM.utils.slam_external import calc_mse, calc_psnr
    b = ec.make_batch((5, 17, 33), 0, "none")
    for v in range(5):
        x, y = _dev(np.clip(b["render"][v], 0, 1), gpu), _dev(b["gt_f32"][v], gpu)
        mse, psnr = calc_mse(x, y), calc_psnr(x, y)
        assert mse.shape == (3, 1) and psnr.shape == (3, 1) and mse.dtype == torch.float32 and mse.is_cuda
        # the reference's two lines, in binary32 and binary64
        m32 = ((x - y) ** 2).view(3, -1).mean(1, keepdim=True)
        m64 = ((x.double() - y.double()) ** 2).view(3, -1).mean(1, keepdim=True)
        p32, p64 = 20 * torch.log10(1.0 / torch.sqrt(m32)), 20 * torch.log10(1.0 / torch.sqrt(m64))
        for c in range(3):
            assert ec.need(mse[c, 0], m32[c, 0], m64[c, 0]) <= 1.0 and ec.need(psnr[c, 0], p32[c, 0], p64[c, 0]) <= 1.0
        if b["families"][v] == "identical":
            assert torch.isinf(psnr).all() and (mse == 0).all()
    # anything else takes the torch expression: the host, another dtype, a gradient
    xc, yc = torch.rand((3, 8, 9)), torch.rand((3, 8, 9))
    assert torch.equal(calc_mse(xc, yc), ((xc - yc) ** 2).view(3, -1).mean(1, keepdim=True)) and calc_psnr(xc, yc).shape == (3, 1)
    xg = x.clone().requires_grad_(True)
    calc_psnr(xg, y).sum().backward()
    assert xg.grad is not None and calc_mse(x[:1], y[:1]).shape == (1, 1)
