"""-m gpu: every entry point under the cameras of tests/cameras.py -- anisotropic focal lengths (tanfovx != tanfovy), an off-centre
principal point, a view matrix that is not the identity, scale modifiers 1.7 and 0.4, a visible background -- on scenes spread over
1.6 x each camera's own frustum (tests/test_camera_cases_cpu.py proves what they exercise).  References and tolerances are those of
the existing test of the same entry point; there is no tolerance of this file's own.

  fr_forward / fr_backward / fr_backward_ws   test_gpu_rasterizer_parity.py (forward bit-exact; backward 1e-4, the arbiter rule for power 2)
  forward_pair / fr_backward_pair / _pair_ws  test_gpu_rasterizer_parity.py::test_fused_rgb_depth_silhouette_pair
  fr_fisher_views                             test_gpu_outh_variants.py (entries 1e-4 + 1e-7 max, scores 1e-4; counts exact)
  fr_render_views                             test_gpu_render_views.py (bit for bit)
  fr_fisher_point_views                       test_gpu_point_scores.py (the entry rule through the weighted sum)
  fr_fisher_pose_views                        test_gpu_pose_fisher.py (1e-4 |H64| + K_POSE 2^-24 JJ)
  GaussianSLAM / GaussianObjectSLAM           test_gpu_fisher_parity.py::test_slam_operator_surface (scores 1e-4)"""
import numpy as np
import pytest
import torch

import cameras as C
from gpu_util import hip_forward, hip_backward, assert_close, to_dev

pytestmark = pytest.mark.gpu

RASTER = C.by_name(C.RASTER_CASES)
BATCHED = C.by_name(C.BATCHED_CASES)
GRAD_NAMES = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations")
ABI_ORDER = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _backward(gpu, cam, fwd, dL, power, segmented):
    """fr_backward_ws with its scratch (segmented: the chunked kernels) or without (the single-pass walk)"""
    from fisher_rast import ops
    t = fwd["tensors"]
    geom, binning, img = fwd["buffers"]
    o = ops.rasterize_backward(t["bg"], t["means3D"], fwd["radii_t"], t["colors"], t["scales"], t["rotations"], cam.scale_modifier, t["cov3D"],
                               t["view"], t["proj"], cam.tanfovx, cam.tanfovy, to_dev(dL, gpu), t["sh"], cam.sh_degree, t["campos"], geom,
                               fwd["num_rendered"], binning, img, power, segmented=segmented)
    torch.cuda.synchronize()
    return {n: x.cpu().numpy() for n, x in zip(ABI_ORDER, o)}


def _assert_forward_bit_exact(got, want):
    """the list of test_gpu_rasterizer_parity.py::test_forward_bit_exact"""
    vis = want["radii"] > 0
    assert vis.sum() > 0
    assert np.array_equal(got["radii"], want["radii"])
    for k in ("depths", "means2D", "conic_opacity", "cov3D"):
        assert np.array_equal(bits(got[k][vis]), bits(want[k][vis])), k
    assert got["num_rendered"] == want["num_rendered"]
    assert np.array_equal(got["ranges"], want["ranges"])
    assert np.array_equal(got["point_list"], want["point_list"])
    assert np.array_equal(got["n_contrib"], want["n_contrib"])
    for k in ("final_T", "color", "depth"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k


# ---- 1. the single-view rasteriser ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def raster(gpu, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            c = RASTER[name]
            cam = C.oracle_camera(oracle, c)
            sc = C.raster_scene(c)
            args = dict(colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])
            want = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], **args)
            got = hip_forward(gpu, cam, sc["means3D"], sc["opacities"], **args)
            cache[name] = dict(c=c, cam=cam, sc=sc, want=want, got=got, grads={})
        return cache[name]
    return get


def _oracle_grads(oracle, r, power):
    """(dL, oracle gradients, arbiter gradients for power 2): once per (case, power)"""
    if power not in r["grads"]:
        cam, sc, want = r["cam"], r["sc"], r["want"]
        H, W = cam.image_height, cam.image_width
        dL = np.random.default_rng(5).normal(size=(3, H, W)).astype(np.float32) if power == 1 else np.full((3, H, W), 1e-3, np.float32)
        gw = oracle.rasterize_backward(cam, want, dL, power)
        ga = None
        if power == 2:
            w64 = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], scales=sc["scales"],
                                           rotations=sc["rotations"], decisions=want)
            ga = oracle.rasterize_backward(cam, w64, dL, power)
        r["grads"][power] = (dL, gw, ga)
    return r["grads"][power]


@pytest.mark.parametrize("name", C.ids(C.RASTER_CASES))
def test_forward_bit_exact(raster, name):
    r = raster(name)
    _assert_forward_bit_exact(r["got"], r["want"])
    if name in C.CHUNKED_CASES:
        assert r["got"]["tile_count"].max() > 256


@pytest.mark.parametrize("segmented", [True, False], ids=["chunked", "single_pass"])
@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("name", C.ids(C.RASTER_CASES))
def test_backward_parity(raster, oracle, gpu, name, power, segmented):
    """the rules of test_gpu_rasterizer_parity.py::test_backward_parity, on fr_backward_ws with and without its scratch (the chunked
    kernels cut lists in the three CHUNKED_CASES; under offcentre-m0.4, whose longest list is 133, they run on single segments)"""
    r = raster(name)
    dL, gw, ga = _oracle_grads(oracle, r, power)
    gg = _backward(gpu, r["cam"], r["got"], dL, power, segmented)
    for n in GRAD_NAMES:
        if power == 2:
            o, a = gw[n].astype(np.float64).reshape(gw[n].shape[0], -1), ga[n].reshape(gw[n].shape[0], -1)
            big = np.abs(a) > 1e-7 * np.abs(a).max()
            rr = np.where(big, np.abs(o - a) / np.maximum(np.abs(a), 1e-300), 0.0).max(axis=1, keepdims=True)
            tol = (1e-4 + np.minimum(1.25 * rr, 0.3)) * np.abs(o) + 1e-7 * np.abs(o).max()
            err = np.abs(gg[n].astype(np.float64).reshape(o.shape) - o)
            print(f"[{name}/p2/{n}] worst |err| / tol {float((err / np.maximum(tol, 1e-300)).max()):.3f}, widened {int((rr > 2e-5).sum())}")
            assert not (err > tol).any(), (f"{name}/{n}", int((err > tol).sum()), float((err / np.maximum(tol, 1e-300)).max()))
            assert (rr > 2e-5).mean() < 0.02
        else:
            assert_close(gg[n], gw[n], 1e-4, f"{name}/{n}", atol_frac=2e-5)
    assert gg["dL_dsh"].shape == (r["sc"]["means3D"].shape[0], 0, 3)


def test_cov3d_precomp_path(gpu, oracle):
    """test_gpu_rasterizer_parity.py::test_cov3d_precomp_path under narrow_wide, modifier 1.7, the rotated view (campos is the
    centre of that view)"""
    c = RASTER["narrow_wide-m1.7"]
    cam = C.oracle_camera(oracle, c)
    assert np.allclose(cam.campos, np.linalg.inv(c.view_w2c.astype(np.float64))[:3, 3], atol=1e-6)
    sc = C.raster_scene(c)
    base = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], scales=sc["scales"], rotations=sc["rotations"])
    cov = base["cov3D"].copy()
    cov[base["radii"] == 0] = [1e-3, 0, 0, 1e-3, 0, 1e-3]          # culled splats never had their covariance computed
    want = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], cov3D_precomp=cov)
    got = hip_forward(gpu, cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], cov3D_precomp=cov)
    vis = want["radii"] > 0
    assert np.array_equal(got["radii"], want["radii"]) and np.array_equal(got["point_list"], want["point_list"])
    assert np.array_equal(bits(got["means2D"][vis]), bits(want["means2D"][vis]))
    assert np.array_equal(bits(got["conic_opacity"][vis]), bits(want["conic_opacity"][vis]))
    assert np.array_equal(bits(got["color"]), bits(want["color"])) and np.array_equal(bits(got["depth"]), bits(want["depth"]))
    dL = np.random.default_rng(1).normal(size=(3, c.H, c.W)).astype(np.float32)
    gw = oracle.rasterize_backward(cam, want, dL, 1)
    gg = hip_backward(gpu, cam, got, dL, 1)
    for n in ("dL_dmeans3D", "dL_dcov3D", "dL_dopacity", "dL_dcolors", "dL_dmeans2D"):
        assert_close(gg[n], gw[n], 1e-4, n, atol_frac=2e-5)
    assert np.all(gg["dL_dscales"] == 0) and np.all(gg["dL_drotations"] == 0)


@pytest.mark.parametrize("power", [1, 2])
def test_sh_degree_3(gpu, oracle, power):
    """test_gpu_rasterizer_parity.py::test_sh_forward / test_sh_backward (degree 3) under offcentre, modifier 0.4, the rotated view:
    the view direction is taken from the campos of that view"""
    c = RASTER["offcentre-m0.4"]
    cam = C.oracle_camera(oracle, c)._replace(sh_degree=3)
    assert np.abs(cam.campos).max() > 0.05
    sc = C.raster_scene(c)
    P, M = sc["means3D"].shape[0], 16
    shs = np.random.default_rng(3).normal(scale=2.0, size=(P, M, 3)).astype(np.float32)   # large enough to clamp some colours
    want = oracle.rasterize_forward(cam, sc["means3D"], sc["opacities"], shs=shs, scales=sc["scales"], rotations=sc["rotations"])
    got = hip_forward(gpu, cam, sc["means3D"], sc["opacities"], shs=shs, scales=sc["scales"], rotations=sc["rotations"])
    vis = want["radii"] > 0
    assert want["clamped"].any()
    assert np.array_equal(bits(got["rgb"][vis]), bits(want["rgb"][vis]))
    assert np.array_equal(got["clamped"][vis], want["clamped"][vis])
    assert np.array_equal(bits(got["color"]), bits(want["color"]))
    dL = np.random.default_rng(7).normal(size=(3, c.H, c.W)).astype(np.float32) if power == 1 else np.full((3, c.H, c.W), 1e-3, np.float32)
    gw = oracle.rasterize_backward(cam, want, dL, power)
    gg = hip_backward(gpu, cam, got, dL, power)
    fl = 2e-5 if power == 1 else 1e-7
    for n in ("dL_dmeans3D", "dL_dcolors", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dmeans2D", "dL_dsh"):
        assert_close(gg[n], gw[n], 1e-4, f"deg3/p{power}/{n}", atol_frac=fl)
    assert np.abs(gg["dL_dsh"]).max() > 0


@pytest.mark.parametrize("name", C.ids(C.RASTER_CASES))
def test_mark_visible(gpu, oracle, name):
    from fisher_rast import ops
    c = RASTER[name]
    cam = C.oracle_camera(oracle, c)
    sc = C.frustum_scene(c, 5000, 12, zmin=-2.0, zmax=3.0)
    want = oracle.mark_visible(cam, sc["means3D"])
    got = ops.mark_visible(to_dev(sc["means3D"], gpu), to_dev(cam.viewmatrix, gpu), to_dev(cam.projmatrix, gpu))
    assert 0 < want.sum() < want.size
    assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), want)


@pytest.fixture(scope="module")
def pair_forwards(gpu, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            c = C.by_name(C.PAIR_CASES)[name]
            cam, sc = C.oracle_camera(oracle, c), C.pair_scene(c)
            rng = np.random.default_rng(23)
            feats = rng.uniform(0, 1, (sc["means3D"].shape[0], 3)).astype(np.float32)
            dL = (rng.normal(size=(3, c.H, c.W)).astype(np.float32), rng.normal(size=(3, c.H, c.W)).astype(np.float32))
            geo = dict(scales=sc["scales"], rotations=sc["rotations"])
            one = hip_forward(gpu, cam, sc["means3D"], sc["opacities"], colors_precomp=sc["colors"], **geo)
            two = hip_forward(gpu, cam, sc["means3D"], sc["opacities"], colors_precomp=feats, **geo)
            cache[name] = (c, cam, sc, feats, dL, one, two)
        return cache[name]
    return get


@pytest.mark.parametrize("segmented", [True, False], ids=["chunked", "tile_kernel"])
@pytest.mark.parametrize("name", C.ids(C.PAIR_CASES))
def test_fused_pair(pair_forwards, gpu, name, segmented):
    """fr_forward_pair / fr_backward_pair(_ws): both images bit-identical to two separate forwards, every shared leaf gradient equal
    to the sum of the two separate backwards and each image's own gradients to its own backward's (the rules of
    test_gpu_rasterizer_parity.py::test_fused_rgb_depth_silhouette_pair).  Both sides add the tiles' partial sums with binary32 atomic
    adds in a run-dependent order; the scenes keep splats that cover the whole image out (tests/cameras.py, PAIR_CASES), with which
    two runs of the same separate backward differ by most of this rule."""
    from fisher_rast import ops
    c, cam, sc, feats, (dLa, dLb), one, two = pair_forwards(name)
    assert (one["radii"] > 0).sum() > 500 and (one["tile_count"] > 600).sum() >= 2      # lists the chunked kernels cut
    t = one["tensors"]
    res = ops.rasterize_forward(t["bg"], t["means3D"], t["colors"], t["opacity"], t["scales"], t["rotations"], cam.scale_modifier, t["cov3D"],
                                t["view"], t["proj"], cam.tanfovx, cam.tanfovy, c.H, c.W, t["sh"], 0, t["campos"], False, features=to_dev(feats, gpu))
    R, color, radii, geom, binning, img, depth, fimg = res
    assert R == one["num_rendered"] and np.array_equal(radii.cpu().numpy(), one["radii"])
    assert np.array_equal(bits(color), bits(one["color"])) and np.array_equal(bits(fimg), bits(two["color"]))
    assert np.array_equal(bits(depth), bits(one["depth"]))
    ga, gb = hip_backward(gpu, cam, one, dLa, 1), hip_backward(gpu, cam, two, dLb, 1)
    o = ops.rasterize_backward_pair(t["bg"], t["means3D"], radii, t["colors"], to_dev(feats, gpu), t["scales"], t["rotations"], cam.scale_modifier,
                                    t["cov3D"], t["view"], t["proj"], cam.tanfovx, cam.tanfovy, to_dev(dLa, gpu), to_dev(dLb, gpu), t["campos"],
                                    geom, binning, img, num_rendered=R, segmented=segmented)
    torch.cuda.synchronize()
    m2, m2f, dc, df, dop, dm3, dcov, dsc, drot = (x.cpu().numpy() for x in o)

    def close(got, want, rtol, what, atol_frac):
        want = np.asarray(want, np.float64)
        worst = float((np.abs(got - want) / (rtol * np.abs(want) + atol_frac * np.abs(want).max())).max())
        print(f"[{name}/{'chunked' if segmented else 'tile_kernel'}] {what}: worst |err| / tol {worst:.3f}")
        assert_close(got, want, rtol, what, atol_frac=atol_frac)
    close(m2, ga["dL_dmeans2D"], 1e-5, "means2D.grad (colour render only)", 1e-7)
    close(m2f, gb["dL_dmeans2D"], 1e-5, "means2D.grad (feature render)", 1e-7)
    close(dc, ga["dL_dcolors"], 1e-4, "pair d/dcolors", 1e-6)
    close(df, gb["dL_dcolors"], 1e-4, "pair d/dfeatures", 1e-6)
    for got, n in ((dop, "dL_dopacity"), (dm3, "dL_dmeans3D"), (dcov, "dL_dcov3D"), (dsc, "dL_dscales"), (drot, "dL_drotations")):
        close(got, ga[n].astype(np.float64) + gb[n].astype(np.float64), 1e-4, f"pair {n}", 1e-6)


def test_autograd_front_end_gives_the_oracles_leaf_gradients(raster, oracle, gpu):
    """GaussianRasterizer under narrow_wide with scale_modifier = 1.7: every leaf gradient is the oracle's backward's -- dL_dscales in
    the reference's convention (backward.cu:429-459 leaves the modifier out of it)."""
    from diff_gaussian_rasterization import GaussianRasterizer, GaussianRasterizationSettings
    r = raster("narrow_wide-m1.7")
    c, cam, sc = r["c"], r["cam"], r["sc"]
    dL, gw, _ = _oracle_grads(oracle, r, 1)
    dev = C.device_camera(c, gpu)
    assert isinstance(dev, GaussianRasterizationSettings) and dev.scale_modifier == 1.7 and dev.tanfovx != dev.tanfovy
    t = {k: torch.tensor(v, device=gpu, requires_grad=True) for k, v in sc.items()}
    op = t["opacities"].reshape(-1, 1)
    m2d = torch.zeros((sc["means3D"].shape[0], 3), device=gpu, requires_grad=True)
    im, radii, depth = GaussianRasterizer(dev)(means3D=t["means3D"], means2D=m2d, opacities=op, colors_precomp=t["colors"],
                                               scales=t["scales"], rotations=t["rotations"])
    assert np.array_equal(bits(im), bits(r["want"]["color"])) and np.array_equal(radii.cpu().numpy(), r["want"]["radii"])
    (im * to_dev(dL, gpu)).sum().backward()
    for leaf, n in ((t["means3D"], "dL_dmeans3D"), (t["colors"], "dL_dcolors"), (t["opacities"], "dL_dopacity"), (t["scales"], "dL_dscales"),
                    (t["rotations"], "dL_drotations"), (m2d, "dL_dmeans2D")):
        assert_close(leaf.grad.cpu().numpy().reshape(gw[n].shape), gw[n], 1e-4, f"autograd {n}", atol_frac=2e-5)


# ---- 2. the view-batched entry points -----------------------------------------------------------------------------------------
KEYS = ("means3D", "colors", "rotations", "opacities", "scales")


@pytest.fixture(scope="module")
def batched(gpu, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            c = BATCHED[name]
            sc = C.batched_scene(c)
            cache[name] = dict(c=c, sc=sc, ocam=C.oracle_camera(oracle, c), cam=C.device_camera(c, gpu), w2cs=C.frustum_poses(c, 3),
                               t=[torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu) for k in KEYS], hess={}, arb={})
        return cache[name]
    return get


def _hess(oracle, b, columns):
    """per view (cur_H, vis_count, num_rendered) of the oracle, once per (case, columns)"""
    if columns not in b["hess"]:
        out = [oracle.compute_hessian(b["ocam"], w, *(b["sc"][k] for k in KEYS), columns=columns, return_all=True) for w in b["w2cs"]]
        b["hess"][columns] = (np.stack([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2]["num_rendered"] for o in out]))
    return b["hess"][columns]


def _scorer(b, columns, **kw):
    from fisher_rast.ops import FisherScorer
    return FisherScorer(b["cam"], *b["t"], columns=columns, **kw)


# (spatial_order with out_H is left to test_gpu_spatial_order.py: two distinct splats of bit-equal depth in one tile -- the blobs of these
# scenes hold tens of such pairs per view -- composite in Z-curve order there, which moves single entries by more than the entry rule)
PATHS = ["scores_fixed", "scores_packed", "scores_general", "scores_spatial", "out_h", "both"]
# (a camera whose view is not the identity is on the general front end anyway: "scores_fixed" is that path there)
FISHER = [(n, p) for n in C.ids(C.BATCHED_CASES) for p in PATHS if not (p == "scores_general" and n.endswith("-rot"))]


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("name,path", FISHER)
def test_fisher_views(batched, oracle, gpu, name, path, columns):
    """fr_fisher_views against oracle.compute_hessian, V = 3 (a small motion, a pose in a corner of the cloud, one outside it)"""
    b = batched(name)
    want, vis, nr = _hess(oracle, b, columns)
    P, V = want.shape[1], len(b["w2cs"])
    w2c = torch.from_numpy(b["w2cs"]).to(gpu)
    kw = dict(tile_capacity=0) if path == "scores_packed" else dict(spatial_order=True) if path == "scores_spatial" else {}
    sc = _scorer(b, columns, **kw)
    assert sc.view_is_identity == (not name.endswith("-rot"))
    if path == "scores_packed":
        assert sc.tile_capacity == 0
    if path == "scores_general":
        sc.view_is_identity = False
    Hi = torch.rand((P, columns), generator=torch.Generator().manual_seed(3)) * 2.0 + 0.05
    out = torch.zeros((V, P, columns), device=gpu) if path in ("out_h", "both") else None
    r = sc.run(w2c, H_inv=None if path == "out_h" else Hi.to(gpu), out_H=out, out_H_per_view=out is not None)
    torch.cuda.synchronize()
    assert np.array_equal(r["vis_count"].cpu().numpy(), vis), (r["vis_count"].cpu().numpy(), vis)
    assert np.array_equal(r["num_rendered"].cpu().numpy(), nr), (r["num_rendered"].cpu().numpy(), nr)
    if out is not None:
        for v in range(V):
            assert_close(out[v].cpu().numpy(), want[v], 1e-4, f"{name}/{path}: cur_H[{v}]", atol_frac=1e-7)
    if r["scores"] is not None:
        ws = (want.astype(np.float64) * Hi.double().numpy()[None]).sum(axis=(1, 2))
        s = r["scores"].cpu().double().numpy()
        assert np.all(np.abs(s - ws) <= 1e-4 * np.abs(ws)), (s, ws)


def test_fisher_views_beyond_4096_tiles(gpu, oracle):
    """test_gpu_outh_variants.py's 1040 x 1040 / P = 3000 scene (the single-view front end, dense records) with fy changed
    (tanfov 1.0 / 1.6), an off-centre principal point and modifier 1.7, 11 columns: the diagonal and the scores.  This is about the
    camera and the modifier beyond 4096 tiles; room_shell is not spread over the frustum (the oracle sees one to three visible clamped
    splats per axis and view), so the clamp is left to the cases above."""
    from fisher_rast import synthetic
    from fisher_rast.ops import FisherScorer
    P, V, W, H, columns = 3000, 2, 1040, 1040, 11
    c = C.Case("wide_y-1040", W, H, ((520.0, 0.0, 500.0), (0.0, 325.0, 560.0), (0.0, 0.0, 1.0)), 1.7, C.BG, np.eye(4, dtype=np.float32))
    act = synthetic.activate(synthetic.room_shell(P, seed=8))
    a = {k: v.numpy() for k, v in act.items()}
    w2cs = synthetic.invert_rigid(synthetic.candidate_poses(V, seed=8))
    ocam = C.oracle_camera(oracle, c)
    res = [oracle.compute_hessian(ocam, w, a["means3D"], a["rgb_colors"], a["rotations"], a["opacities"], a["scales"], columns=columns,
                                  return_all=True) for w in w2cs.numpy()]
    want = np.stack([o[0] for o in res])
    sc = FisherScorer(C.device_camera(c, gpu), *(act[k].to(gpu) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")), columns=columns)
    assert sc.tiles == 65 * 65
    out = torch.zeros((V, P, columns), device=gpu)
    r = sc.run(w2cs.to(gpu), out_H=out, out_H_per_view=True)
    assert np.array_equal(r["vis_count"].cpu().numpy(), [o[1] for o in res])
    assert np.array_equal(r["num_rendered"].cpu().numpy(), [o[2]["num_rendered"] for o in res])
    for v in range(V):
        assert_close(out[v].cpu().numpy(), want[v], 1e-4, f"4225 tiles: cur_H[{v}]", atol_frac=1e-7)
    Hi = torch.rand((P, columns), generator=torch.Generator().manual_seed(5)) * 2.0 + 0.05
    s = sc.run(w2cs.to(gpu), H_inv=Hi.to(gpu))["scores"].cpu().double().numpy()
    ws = (want.astype(np.float64) * Hi.double().numpy()[None]).sum(axis=(1, 2))
    assert np.all(np.abs(s - ws) <= 1e-4 * np.abs(ws)), (s, ws)


@pytest.mark.parametrize("name", C.ids(C.BATCHED_CASES))
def test_render_views(batched, oracle, gpu, name):
    """fr_render_views: colour, (z, 1, z z), median depth and final_T of every view against the oracle's two forwards, bit for bit
    (test_gpu_render_views.py::_same_view), the background in C + T bg"""
    b = batched(name)
    sc, ocam = b["sc"], b["ocam"]
    got = {k: v.cpu().numpy() for k, v in _scorer(b, 4).render_views(torch.from_numpy(b["w2cs"]).to(gpu)).items()}
    geo = dict(scales=sc["scales"], rotations=sc["rotations"])
    clear = []
    for v, w in enumerate(b["w2cs"]):
        m = oracle.transform_points(w, sc["means3D"])
        rgb = oracle.rasterize_forward(ocam, m, sc["opacities"], colors_precomp=sc["colors"], **geo)
        z = m[:, 2].astype(np.float32)
        ds = oracle.rasterize_forward(ocam, m, sc["opacities"], colors_precomp=np.stack([z, np.ones_like(z), z * z], 1), **geo)
        assert (rgb["radii"] > 0).sum() > 0
        clear.append(bool((rgb["final_T"] > 0.5).any()))
        assert np.array_equal(bits(got["render"][v]), bits(rgb["color"])), (name, v, "render")
        assert np.array_equal(bits(got["median_depth"][v]), bits(rgb["depth"])), (name, v, "median depth")
        assert np.array_equal(bits(got["final_T"][v]), bits(rgb["final_T"])), (name, v, "final_T")
        assert np.array_equal(bits(got["depth_sil"][v]), bits(ds["color"])), (name, v, "depth_sil")
        assert int(got["vis_count"][v]) == int((rgb["radii"] > 0).sum()) and int(got["num_rendered"][v]) == int(rgb["num_rendered"])
    assert any(clear)                                                  # the background shows in some view


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("name", C.ids(C.BATCHED_CASES))
def test_point_views(batched, oracle, gpu, name, columns):
    """fr_fisher_point_views: point[v, i] and the view scores against sum_c cur_H H_inv of the oracle, with the bounds of
    test_gpu_point_scores.py::test_point_scores_against_the_oracle; point_max is the maximum over the views, bit for bit"""
    from scenes import rel_err
    from test_gpu_point_scores import _want_tol, _check
    from test_gpu_scorer_adversarial import _entry_tolerance
    b = batched(name)
    if columns not in b["arb"]:
        cur = [oracle.compute_hessian(b["ocam"], w, *(b["sc"][k] for k in KEYS), columns=columns, arbiter=True) for w in b["w2cs"]]
        cur_o, cur_a = np.stack([h for h, _, _ in cur]), np.stack([h for _, h, _ in cur])
        H_inv_o = (np.float32(1.0) / (cur_o[1:].sum(0, dtype=np.float32) + np.float32(0.1))).astype(np.float32)
        ent = [_entry_tolerance(cur_o[v], cur_a[v], columns) for v in range(len(cur))]
        b["arb"][columns] = dict(cur_o=cur_o, cur_a=cur_a, vis_o=np.array([v for _, _, v in cur]), H_inv_o=H_inv_o,
                                 tol_entry=np.stack([e[0] for e in ent]), r_G=np.stack([e[1] for e in ent]))
    ref = b["arb"][columns]
    V, P = ref["cur_o"].shape[:2]
    want, tol = _want_tol(ref, ref["H_inv_o"])
    assert int((ref["r_G"] > 2e-5).sum()) <= 0.02 * V * P
    r = _scorer(b, columns).point_scores(torch.from_numpy(b["w2cs"]).to(gpu), torch.from_numpy(ref["H_inv_o"]).to(gpu))
    got = r["point_scores"].cpu().numpy().astype(np.float64)
    print(f"[{name}-{columns}] worst |err| / tol {float((np.abs(got - want) / tol).max()):.3f}")
    assert np.array_equal(r["vis_count"].cpu().numpy(), ref["vis_o"])
    _check(got, want, tol, (name, columns))
    assert rel_err(r["scores"].cpu().numpy().astype(np.float64), want.sum(1)) < 1e-4
    assert np.array_equal(r["point_max"].cpu().numpy(), r["point_scores"].cpu().numpy().max(0))


@pytest.mark.parametrize("name", C.ids(C.POSE_CASES))
def test_pose_views(oracle, gpu, name):
    """fr_fisher_pose_views against pose_fisher_ref.pose_hessian_ref with the rule and the constant of test_gpu_pose_fisher.py, under
    48 x 32 variants of an off-centre and a rotated anisotropic case (modifier 1.7)"""
    import pose_fisher_ref as pf
    from fisher_rast.ops import FisherScorer
    from test_gpu_pose_fisher import _check
    c = C.by_name(C.POSE_CASES)[name]
    sc, w2cs = C.pose_scene(c), C.pose_views(c)
    s = FisherScorer(C.device_camera(c, gpu), *(torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu) for k in KEYS))
    got = s.pose_fisher(torch.from_numpy(w2cs).to(gpu)).cpu().numpy()
    assert got.shape == (len(w2cs), 6, 6) and np.isfinite(got).all()
    ocam = C.oracle_camera(oracle, c)
    for v, w in enumerate(w2cs):
        H64, JJ, _ = pf.pose_hessian_ref(ocam, w, sc)
        assert np.abs(H64).max() > 0
        _check(got[v], H64, JJ, f"{name} view {v}")
        assert np.array_equal(got[v], got[v].T)


# ---- 3. the SLAM layer hands K through unchanged --------------------------------------------------------------------------------
@pytest.mark.parametrize("cls_name,columns", [("GaussianSLAM", 4), ("GaussianObjectSLAM", 11)])
def test_slam_layer_with_non_unit_intrinsics(oracle, gpu, cls_name, columns):
    """test_gpu_fisher_parity.py::test_slam_operator_surface with the off-centre anisotropic K: H_train 1e-4 + 1e-7 max, scores 1e-4"""
    import models.gaussian_slam as mgs
    from scenes import rel_err
    c = BATCHED["offcentre-m1.7"]
    sc = C.batched_scene(c)
    params = dict(means3D=sc["means3D"], rgb_colors=sc["colors"], unnorm_rotations=sc["rotations"] * 2.0,
                  logit_opacities=np.log(sc["opacities"] / (1 - sc["opacities"])).reshape(-1, 1), log_scales=np.log(sc["scales"]))
    params = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in params.items()}
    slam = getattr(mgs, cls_name)(params={k: v.clone() for k, v in params.items()}, intrinsics=np.asarray(c.K), width=c.W, height=c.H, device=gpu)
    # the activated map the surface builds (gaussian.py:1529-1533); the surface's camera has modifier 1 and a black background
    args = (sc["means3D"], sc["colors"], torch.nn.functional.normalize(params["unnorm_rotations"]).numpy(),
            torch.sigmoid(params["logit_opacities"]).numpy().reshape(-1), torch.exp(params["log_scales"]).numpy())
    ocam = oracle.setup_camera(c.W, c.H, c.K, np.eye(4))
    w2cs = C.frustum_poses(c, 5)
    kf, cand = w2cs[3:], w2cs[:3]
    for w in kf:
        slam.add_keyframe(w)
    H_train = slam.compute_H_train()
    H_train_o = oracle.compute_h_train(ocam, kf, *args, columns=columns)
    assert_close(H_train.cpu().numpy(), H_train_o, 1e-4, "H_train", atol_frac=1e-7)
    poses = [torch.linalg.inv(torch.from_numpy(w).double()).float().to(gpu) for w in cand]
    scores, c2ws = slam.pose_eval(poses, random_gaussian_params=None)
    w2c_dev = torch.linalg.inv(torch.stack(poses)).cpu().numpy()
    want, _ = oracle.pose_eval(ocam, w2c_dev, H_train_o, *args, columns=columns)
    assert scores.shape == (3,) and rel_err(scores.numpy(), want) < 1e-4, (scores, want)
