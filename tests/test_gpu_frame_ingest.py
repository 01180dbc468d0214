"""-m gpu: the frame ingest (fr_frame_ingest_select / fr_frame_ingest_emit, csrc/fr_ingest.hip) and what is written on it
(get_pointcloud / add_new_gaussians of models/SLAM/gaussian.py).

Through the C ABI on guarded buffers, for every family and shape of tests/ingest_cases.py: median bits, index list, count and every
emitted row against the g++ harness over the same header -- bits, except the log scales (logf is the platform's), which are held to
the binary64 value by the CPU test's rule.  The product functions against the reference-order torch chain run on the device, and no
host synchronisation inside either call."""
import ctypes

import numpy as np
import pytest
import torch

import ingest_cases as ic
import scenes

pytestmark = pytest.mark.gpu

GUARD = 64                    # words behind every buffer
GUARD_BITS = 0x5A5A5A5A
OFFSET = 2                    # rows in front of the emitted ones


@pytest.fixture(scope="module")
def ingest_harness():
    return ic.build_harness()


class _Guarded:
    """a device buffer of n 32-bit words, filled with the guard pattern, with GUARD more words behind it"""

    def __init__(self, n, dev):
        self.buf = torch.full((n + GUARD,), GUARD_BITS, dtype=torch.int32, device=dev)
        self.n = n

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, dtype=np.uint32):
        return self.buf[:self.n].cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.buf[self.n:] == GUARD_BITS).all())

    def untouched(self):
        return bool((self.buf == GUARD_BITS).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _select(dev, c, mask_in=None, obj_mask=None):
    """fr_frame_ingest_select on guarded status and workspace; (status [5] uint32, idx, pooled, guards intact, workspace).
    mask_in: the mask itself (FR_INGEST_MASK); obj_mask: bytes ANDed into the predicate (FR_INGEST_NONPRESENCE)"""
    from fisher_rast import _lib
    lib = _lib.load()
    H, W, d = c["H"], c["W"], c["d"]
    G = (H // d) * (W // d)
    nws = int(lib.fr_frame_ingest_workspace_bytes(H, W, d))
    assert nws >= _lib.FR_INGEST_WS_INDEX_OFFSET + 5 * G and nws % 4 == 0
    status, ws = _Guarded(_lib.FR_INGEST_STATUS_WORDS, dev), _Guarded(nws // 4, dev)
    cfg = _lib.FrameIngestCfg(H, W, d, _lib.FR_INGEST_NONPRESENCE if mask_in is None else _lib.FR_INGEST_MASK, ic.SIL_THRES, c["ratio"],
                              1, 3, 3, 3, None)
    ds, gt = _dev(c["depth_sil"], dev), _dev(c["gt"], dev)
    given = mask_in if mask_in is not None else obj_mask
    m = None if given is None else _dev(np.ascontiguousarray(given, np.uint8), dev)
    _lib.check(lib.fr_frame_ingest_select(ctypes.byref(cfg), ds.data_ptr() if mask_in is None else None, gt.data_ptr() if mask_in is None else None,
                                          None if m is None else m.data_ptr(), status.ptr, ws.ptr, nws, _stream(dev)), "fr_frame_ingest_select")
    torch.cuda.synchronize()
    st = status.get()
    words = ws.get()
    o = _lib.FR_INGEST_WS_INDEX_OFFSET // 4
    idx = words[o:o + int(st[0])].view(np.int32).copy()
    pooled = words[o + G:].view(np.uint8)[:G].astype(bool)
    return st, idx, pooled, status.intact() and ws.intact(), ws


def _emit(dev, c, ws, count, transform_pts=True, scale_cols=3, row_offset=OFFSET):
    """fr_frame_ingest_emit into guarded destinations of row_offset + count rows; (dict of uint32 arrays, every guard intact,
    whether nothing at all was written)"""
    from fisher_rast import _lib
    lib = _lib.load()
    rows = row_offset + count
    K, w2c = _dev(c["K"], dev), _dev(c["w2c"], dev)
    color, gt = _dev(c["color"], dev), _dev(c["gt"], dev)
    cols = dict(means=3, rgb=3, rot=4, opac=1, log_scales=scale_cols, msd=1)
    out = {k: _Guarded(rows * n, dev) for k, n in cols.items()}
    cfg = _lib.FrameIngestCfg(c["H"], c["W"], c["d"], 0, 0.0, 0.0, int(transform_pts), scale_cols, 3, 3, K.data_ptr())
    _lib.check(lib.fr_frame_ingest_emit(ctypes.byref(cfg), color.data_ptr(), gt.data_ptr(), w2c.data_ptr(), None if ws is None else ws.ptr,
                                        count, row_offset, *(out[k].ptr for k in ("means", "rgb", "rot", "opac", "log_scales", "msd")),
                                        _stream(dev)), "fr_frame_ingest_emit")
    torch.cuda.synchronize()
    res = {k: out[k].get().reshape(rows, n) for k, n in cols.items()}
    return res, all(g.intact() for g in out.values()), all(g.untouched() for g in out.values())


def _check_rows(got, want, count, tag, row_offset=OFFSET):
    """emitted rows against the harness: bits, the log scales by the rule; the rows in front still hold the guard pattern"""
    for k in ("means", "rgb", "rot", "opac", "msd"):
        w = want[k].reshape(row_offset + count, -1)
        if k == "opac":
            w = np.zeros_like(w)
        assert np.array_equal(got[k][row_offset:], ic.bits(w)[row_offset:]), (tag, k)
        assert np.all(got[k][:row_offset] == GUARD_BITS), (tag, k, "rows in front")
    ls = got["log_scales"].view(np.float32)
    with np.errstate(divide="ignore"):
        want64 = np.log(np.sqrt(want["msd"][row_offset:]).astype(np.float64))
    for col in range(ls.shape[1]):
        assert ic.log_scale_ok(ls[row_offset:, col], want64), (tag, "log_scales", col)
    assert np.all(got["log_scales"][:row_offset] == GUARD_BITS), tag


@pytest.mark.parametrize("case", ic.ALL_CASES, ids=ic.case_id)
def test_kernels_are_the_harness(gpu, ingest_harness, case):
    c = ic.make_case(*case)
    G = (c["H"] // c["d"]) * (c["W"] // c["d"])
    want = ic.harness_select(ingest_harness, c)
    st, idx, pooled, intact, ws = _select(gpu, c)
    assert intact, case
    assert int(st[4]) == want["median_bits"] and int(st[1]) == want["has_nan"] and int(st[2]) == 0 and int(st[3]) == 0, (case, st, want["median_bits"])
    assert int(st[0]) == want["count"] and np.array_equal(pooled, want["pooled"]) and np.array_equal(idx, want["idx"]), case
    st2, idx2, pooled2, _, _ = _select(gpu, c)
    assert np.array_equal(st, st2) and np.array_equal(idx, idx2) and np.array_equal(pooled, pooled2), (case, "second call")
    # the rows, in front of which OFFSET rows stay as they were; isotropic for every other family
    cols = 1 if ic.FAMILIES.index(case[0]) % 2 else 3
    got, intact, untouched = _emit(gpu, c, ws, want["count"], True, cols)
    assert intact, case
    if want["count"] == 0:
        assert untouched, (case, "a count of 0 wrote something")
    else:
        _check_rows(got, ic.harness_emit(ingest_harness, c, want["idx"], True, cols, OFFSET), want["count"], case)
        again, _, _ = _emit(gpu, c, ws, want["count"], True, cols)
        assert all(np.array_equal(got[k], again[k]) for k in got), (case, "second call")
        got, intact, _ = _emit(gpu, c, ws, want["count"], False, 3)
        assert intact, case
        _check_rows(got, ic.harness_emit(ingest_harness, c, want["idx"], False, 3, OFFSET), want["count"], (case, "camera frame"))
    # mask=None: every cell, no index list
    got, intact, _ = _emit(gpu, c, None, G, True, 3, 0)
    assert intact, case
    _check_rows(got, ic.harness_emit(ingest_harness, c, None, True, 3, 0), G, (case, "all cells"), 0)
    rng = np.random.default_rng(G)
    # the object mask of the object-aware module, ANDed into the predicate
    obj = rng.uniform(size=(c["H"], c["W"])) < 0.5
    wo = ic.harness_select(ingest_harness, c, obj_mask=obj)
    st, idx, pooled, intact, _ = _select(gpu, c, obj_mask=obj)
    assert intact and int(st[0]) == wo["count"] and int(st[4]) == want["median_bits"] and int(st[1]) == want["has_nan"], (case, "object mask")
    assert np.array_equal(idx, wo["idx"]) and np.array_equal(pooled, wo["pooled"]), (case, "object mask")
    # the caller's mask
    for m in (rng.uniform(size=(c["H"], c["W"])) < 0.3, np.zeros((c["H"], c["W"]), bool)):
        wm = ic.harness_select(ingest_harness, c, m)
        st, idx, pooled, intact, ws = _select(gpu, c, m)
        assert intact and int(st[0]) == wm["count"] and int(st[1]) == 0 and int(st[4]) == 0, (case, "mask mode")
        assert np.array_equal(idx, wm["idx"]) and np.array_equal(pooled, wm["pooled"]), (case, "mask mode")
    _, intact, untouched = _emit(gpu, c, ws, 0)
    assert intact and untouched, (case, "a count of 0 wrote something")


def test_a_downsample_that_does_not_divide_is_einval(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    assert lib.fr_frame_ingest_workspace_bytes(5, 8, 2) == 0 and lib.fr_frame_ingest_workspace_bytes(8, 5, 2) == 0
    assert lib.fr_frame_ingest_workspace_bytes(8, 6, 2) > 0
    ws = torch.zeros(1 << 14, dtype=torch.int32, device=gpu)
    status = torch.zeros(5, dtype=torch.int32, device=gpu)
    img = torch.zeros((3, 5, 8), device=gpu)
    for H, W in ((5, 8), (8, 5)):
        cfg = _lib.FrameIngestCfg(H, W, 2, _lib.FR_INGEST_NONPRESENCE, 0.5, 2.0, 1, 3, 3, 3, img.data_ptr())
        rc = lib.fr_frame_ingest_select(ctypes.byref(cfg), img.data_ptr(), img.data_ptr(), None, status.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream(gpu))
        assert rc == _lib.FR_EINVAL and b"downsample must divide" in lib.fr_last_error()
        rc = lib.fr_frame_ingest_emit(ctypes.byref(cfg), img.data_ptr(), img.data_ptr(), img.data_ptr(), None, 0, 0, *([None] * 6), _stream(gpu))
        assert rc == _lib.FR_EINVAL and b"divide" in lib.fr_last_error()
    torch.cuda.synchronize()
    assert not status.any() and not ws.any()
    with pytest.raises(_lib.FisherRastError):
        from models.SLAM.gaussian import get_pointcloud
        get_pointcloud(img, img[:1], torch.eye(3, device=gpu), torch.eye(4, device=gpu), downsample=2)


def _case_on_device(c, dev):
    return _dev(c["color"], dev), _dev(c["gt"], dev), _dev(c["K"], dev), _dev(c["w2c"], dev)


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("downsample", [1, 4])
@pytest.mark.parametrize("transform_pts", [True, False], ids=["world", "camera"])
def test_get_pointcloud_against_the_torch_chain(gpu, transform_pts, downsample, with_mask):
    """the same rows in the same order, colours and mean3_sq_dist identical, points by the K rule; with and without mean3_sq_dist"""
    from models.SLAM.gaussian import get_pointcloud
    c = ic.make_case("half", (48, 64, downsample), which_camera=1)
    color, gt, K, w2c = _case_on_device(c, gpu)
    mask = ic.torch_non_presence(_dev(c["depth_sil"], gpu), gt, ic.SIL_THRES, c["ratio"])[0] if with_mask else None
    want_cld, want_msd, _, _ = ic.torch_pointcloud(color, gt, K, w2c, transform_pts, downsample, mask)
    cld, msd = get_pointcloud(color, gt, K, w2c, transform_pts=transform_pts, downsample=downsample, mask=mask, compute_mean_sq_dist=True)
    only = get_pointcloud(color, gt, K, w2c, transform_pts=transform_pts, downsample=downsample, mask=mask)
    assert cld.shape == want_cld.shape and msd.shape == want_msd.shape and cld.dtype == torch.float32
    assert torch.equal(only.view(torch.int32), cld.view(torch.int32))
    assert torch.equal(cld[:, 3:].view(torch.int32), want_cld[:, 3:].contiguous().view(torch.int32))
    assert torch.equal(msd.view(torch.int32), want_msd.contiguous().view(torch.int32))
    idx = None if mask is None else ic.np_select(c)["idx"]
    assert idx is None or len(idx) == cld.shape[0]
    need, chain_need = ic.points_need(cld[:, :3].cpu().numpy(), c, idx, transform_pts), ic.points_need(want_cld[:, :3].cpu().numpy(), c, idx, transform_pts)
    print(f"get_pointcloud points: K needed {need:.2f} (the torch chain on the device: {chain_need:.2f}), K used {ic.K_POINTS}")
    assert need <= ic.K_POINTS
    # a mask that selects nothing: every point, as the reference does
    if with_mask:
        none = get_pointcloud(color, gt, K, w2c, transform_pts=transform_pts, downsample=downsample, mask=torch.zeros_like(mask))
        assert none.shape[0] == (48 // downsample) * (64 // downsample)


def _map_and_frame(dev, isotropic, P=2000, H=48, W=64):
    """a 2k-Gaussian map in front of the first camera, a trajectory of two poses and an RGB-D frame at the second"""
    from models.SLAM.utils.recon_helpers import setup_camera
    sc = scenes.random_scene(P, 21, zmin=1.0, zmax=4.0, spread=0.7, scale=0.08)
    rng = np.random.default_rng(22)
    ls = np.log(sc["scales"])
    params = dict(means3D=sc["means3D"], rgb_colors=sc["colors"], unnorm_rotations=sc["rotations"],
                  logit_opacities=np.log(sc["opacities"] / (1 - sc["opacities"]))[:, None], log_scales=ls[:, :1] if isotropic else ls)
    q = np.array([1.0, 0.01, 0.04, -0.02], np.float32) * 1.7             # not normalised
    params["cam_unnorm_rots"] = np.stack([np.array([1.0, 0, 0, 0], np.float32), q], -1)[None]
    params["cam_trans"] = np.stack([np.zeros(3, np.float32), np.array([0.05, -0.03, 0.02], np.float32)], -1)[None]
    params = {k: torch.nn.Parameter(torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev).requires_grad_(True)) for k, v in params.items()}
    variables = {k: torch.ones(P, device=dev) for k in ("max_2D_radius", "means2D_gradient_accum", "denom")}
    variables["timestep"] = torch.zeros(P, device=dev)
    # a field of view wider than the map (x / z, y / z within 0.7): no silhouette along the borders
    K = np.array([[0.4 * W, 0, 0.45 * W], [0, 0.45 * H, 0.55 * H], [0, 0, 1]], np.float32)
    gt = rng.uniform(0.8, 3.0, (1, H, W)).astype(np.float32)
    gt[0, :3, :] = 0.0
    curr = dict(cam=setup_camera(W, H, K, np.eye(4), device=dev), w2c=torch.eye(4, device=dev), depth=_dev(gt, dev),
                im=_dev(rng.uniform(0, 1, (3, H, W)).astype(np.float32), dev), intrinsics=_dev(K, dev))
    return params, variables, curr


@pytest.mark.parametrize("isotropic", [False, True], ids=["aniso", "iso"])
@pytest.mark.parametrize("downsample", [1, 4])
def test_add_new_gaussians_against_the_torch_chain(gpu, downsample, isotropic):
    from diff_gaussian_rasterization import GaussianRasterizer
    from models.SLAM import gaussian as G
    params, variables, curr = _map_and_frame(gpu, isotropic)
    old = {k: v.detach().clone() for k, v in params.items()}
    P, H, W = 2000, 48, 64
    renders = []

    class Recording(GaussianRasterizer):
        def forward(self, *a, **k):
            out = super().forward(*a, **k)
            renders.append(out[0].detach().clone())
            return out

    add = G.make_add_new_gaussians(G._transform_to_frame, Recording)
    ratio, time_idx, sil_thres = 1.5, 1, 0.5
    out_params, out_vars = add(dict(isotropic=isotropic), params, variables, curr, sil_thres, time_idx, "projective",
                               dict(depth_error_ratio=ratio), add_rand_gaussians=False, downsample_pcd=downsample)
    assert out_params is params and out_vars is variables and len(renders) == 1
    # the same chain, fed the same render
    depth_sil = renders[0]
    mask, _ = ic.torch_non_presence(depth_sil, curr["depth"], sil_thres, ratio)
    w2c = G.frame_w2c(old, time_idx)
    cld, msd, _, _ = ic.torch_pointcloud(curr["im"], curr["depth"], curr["intrinsics"], w2c, True, downsample, mask)
    n = int(cld.shape[0])
    assert 0 < n <= (H // downsample) * (W // downsample) and (downsample > 1 or n < H * W)
    total = P + n
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        t = params[k]
        assert isinstance(t, torch.nn.Parameter) and t.requires_grad and t.is_contiguous() and t.shape[0] == total and t.dtype == torch.float32, k
        assert torch.equal(t[:P].detach().view(torch.int32), old[k].view(torch.int32)), (k, "old rows")
    for k in ("cam_unnorm_rots", "cam_trans"):
        assert torch.equal(params[k].detach(), old[k])
    assert params["log_scales"].shape[1] == (1 if isotropic else 3)
    new = {k: params[k][P:].detach() for k in params if k.startswith(("means", "rgb", "unnorm", "logit", "log_"))}
    assert torch.equal(new["rgb_colors"].contiguous().view(torch.int32), cld[:, 3:].contiguous().view(torch.int32))
    assert bool((new["unnorm_rotations"] == torch.tensor([1.0, 0, 0, 0], device=gpu)).all()) and not bool(new["logit_opacities"].any())
    with np.errstate(divide="ignore"):
        want64 = np.log(np.sqrt(msd.cpu().numpy()).astype(np.float64))
    for col in range(new["log_scales"].shape[1]):
        assert ic.log_scale_ok(new["log_scales"][:, col].cpu().numpy(), want64)
    c = dict(color=curr["im"].cpu().numpy(), gt=curr["depth"].cpu().numpy(), K=curr["intrinsics"].cpu().numpy(), w2c=w2c.cpu().numpy(), d=downsample, H=H, W=W)
    pooled = ic.np_pool(mask.cpu().numpy().reshape(H, W), downsample).reshape(-1)
    need = ic.points_need(new["means3D"].cpu().numpy(), c, np.flatnonzero(pooled))
    print(f"add_new_gaussians points: K needed {need:.2f}, K used {ic.K_POINTS}")
    assert need <= ic.K_POINTS
    for k in ("means2D_gradient_accum", "denom", "max_2D_radius"):
        assert variables[k].shape == (total,) and not bool(variables[k].any())
    assert variables["timestep"].shape == (total,) and not bool(variables["timestep"][:P].any()) and bool((variables["timestep"][P:] == time_idx).all())
    # a frame without a measured depth, then a frame the enlarged map explains: its own render as the measured depth and nothing
    # under the silhouette threshold.  Both return what they were given.
    before, before_vars = dict(params), dict(variables)
    for depth_of, thres in ((lambda: torch.zeros_like(curr["depth"]), sil_thres), (lambda: renders[-1][0:1].clone(), -1.0)):
        p2, v2 = add(dict(isotropic=isotropic), params, variables, dict(curr, depth=depth_of()), thres, time_idx, "projective",
                     dict(depth_error_ratio=ratio), add_rand_gaussians=False, downsample_pcd=downsample)
        assert p2 is params and v2 is variables
        assert all(params[k] is before[k] for k in before) and all(variables[k] is before_vars[k] for k in before_vars)
    assert len(renders) == 3


@pytest.mark.parametrize("downsample", [1, 4])
def test_object_module_add_new_gaussians_keeps_to_the_object_mask(gpu, downsample):
    """object_mask=True is gaussian_object.py's add_new_gaussians: new Gaussians only where curr_data['obj_mask_2d'] is set; the
    same rows as the object module's chain on the same render.  Without the flag the entry is ignored, as gaussian.py ignores it."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from models.SLAM import gaussian as G
    P, H, W, ratio, sil_thres = 2000, 48, 64, 1.5, 0.5
    obj = torch.zeros((H, W), dtype=torch.bool, device=gpu)
    obj[5:30, 10:64] = True
    counts = {}
    for flag in (True, False):
        params, variables, curr = _map_and_frame(gpu, False)
        curr["obj_mask_2d"] = obj.float()                      # not bool: the reference converts, and so must the front end
        add = G.make_add_new_gaussians(G._transform_to_frame, GaussianRasterizer, object_mask=flag)
        add(dict(isotropic=False), params, variables, curr, sil_thres, 1, "projective", dict(depth_error_ratio=ratio),
            add_rand_gaussians=False, downsample_pcd=downsample)
        pts = G._transform_to_frame(params, 1, False, False)[:P]
        old = {k: (v[:P] if v.shape[0] == params["means3D"].shape[0] else v) for k, v in params.items()}
        from models.SLAM.utils.slam_helpers import transformed_params2depthplussilhouette
        depth_sil, _, _ = GaussianRasterizer(raster_settings=curr["cam"])(**transformed_params2depthplussilhouette(old, curr["w2c"], pts))
        mask, _ = ic.torch_non_presence(depth_sil.detach(), curr["depth"], sil_thres, ratio, obj if flag else None)
        cld, msd, _, _ = ic.torch_pointcloud(curr["im"], curr["depth"], curr["intrinsics"], G.frame_w2c(params, 1), True, downsample, mask)
        n = counts[flag] = int(params["means3D"].shape[0]) - P
        assert n == cld.shape[0] and n > 0
        assert torch.equal(params["rgb_colors"][P:].detach().contiguous().view(torch.int32), cld[:, 3:].contiguous().view(torch.int32))
        assert torch.allclose(params["means3D"][P:].detach(), cld[:, :3], rtol=1e-5, atol=1e-5)
    assert counts[True] < counts[False]


def test_random_gaussians_go_behind_the_frames_rows(gpu):
    from models.SLAM import gaussian as G
    params, variables, curr = _map_and_frame(gpu, False)
    ref_params, ref_vars, _ = _map_and_frame(gpu, False)
    G.add_new_gaussians(dict(isotropic=False), ref_params, ref_vars, curr, 0.5, 1, "projective", dict(depth_error_ratio=1.5), add_rand_gaussians=False)
    G.add_new_gaussians(dict(isotropic=False), params, variables, curr, 0.5, 1, "projective", dict(depth_error_ratio=1.5))
    n = int(ref_params["means3D"].shape[0])
    extra = int(params["means3D"].shape[0]) - n
    assert 0 < extra <= 200 and variables["timestep"].shape[0] == n + extra and bool((variables["timestep"][2000:] == 1).all())
    for k in ("means3D", "rgb_colors", "unnorm_rotations", "logit_opacities", "log_scales"):
        assert torch.equal(params[k][:n].detach().view(torch.int32), ref_params[k].detach().view(torch.int32)), k
    assert torch.allclose(params["log_scales"][n:].detach(), torch.full((extra, 3), float(np.log(np.sqrt(0.5))), device=gpu))


def test_no_host_synchronisation_inside_select_and_emit(gpu):
    from fisher_rast import ops
    from models.SLAM.gaussian import get_pointcloud
    c = ic.make_case("half", (48, 64, 4))
    color, gt, K, w2c = _case_on_device(c, gpu)
    depth_sil = _dev(c["depth_sil"], gpu)
    K_host, w2c_host = torch.from_numpy(c["K"]), c["w2c"]                    # host-side camera data must not synchronise either
    means = torch.zeros((200, 3), device=gpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        status, ws = ops.frame_ingest_select(depth_sil, gt, downsample=4, sil_thres=ic.SIL_THRES, depth_error_ratio=c["ratio"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    count = int(status[0])                                                   # the one host read, outside
    assert count == ic.np_select(c)["count"] and 0 < count <= 200
    torch.cuda.set_sync_debug_mode("error")
    try:
        ops.frame_ingest_emit(color, gt, K_host, w2c_host, ws, count, downsample=4, means3D=means)
        cld, msd = get_pointcloud(color, gt, K, w2c, downsample=4, compute_mean_sq_dist=True)
        cld_host_camera = get_pointcloud(color, gt, K_host, w2c_host, downsample=4)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert cld.shape == (12 * 16, 6) and torch.equal(cld, cld_host_camera) and bool(means[:count].any()) and not bool(means[count:].any())
    idx = torch.from_numpy(ic.np_select(c)["idx"].astype(np.int64)).to(gpu)
    assert torch.equal(means[:count], cld[idx, :3])
