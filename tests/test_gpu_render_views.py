"""-m gpu: the batched render (fr_render_views / FisherScorer.render_views / GaussianSLAM.render_at_poses) against the oracle and
against the single-view GPU rasteriser.  Every image is compared as uint32 bits: view v is exactly what the single-view rasteriser
gives for the camera-frame means m = transform_points(w2c_v, means) -- colour, the composited (z, 1, z z), median depth, final
transmittance -- and the counts are the oracle's.  There are no tolerances in this file."""
import numpy as np
import pytest
import torch

from gpu_util import hip_forward
from scenes import random_scene, intrinsics

pytestmark = pytest.mark.gpu

BG = np.array([0.2, 0.5, 0.1], np.float32)          # a background that shows in C + T bg
CASES = ["general", "ragged", "crowded_tile", "ties", "opaque"]
IMAGES = ("render", "depth_sil", "median_depth", "final_T")


def bits(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pose(yaw=0.3, t=(0.2, -0.1, 0.3)):
    w2c = np.eye(4, dtype=np.float32)
    c, s = np.cos(yaw), np.sin(yaw)
    w2c[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    w2c[:3, 3] = t
    return w2c


def _scene(case):
    """the five families of tests/test_gpu_rasterizer_parity.py (same constants), with their own pose"""
    if case == "general":
        W, H, P = 256, 256, 20000
        sc = random_scene(P, 0, zmin=-0.5, zmax=8.0, spread=1.5, scale=0.04)
        sc["means3D"][:40, 2] = np.random.default_rng(0).uniform(0.0011, 0.2, 40)
        w2c = _pose()
    elif case == "ragged":
        W, H, P = 200, 120, 6000
        sc = random_scene(P, 1, scale=0.06)
        w2c = _pose(-0.2)
    elif case == "crowded_tile":
        W, H, P = 64, 64, 9000
        rng = np.random.default_rng(2)
        sc = random_scene(P, 2, scale=0.01)
        z = rng.uniform(1.0, 6.0, P).astype(np.float32)
        sc["means3D"] = np.stack([rng.uniform(-0.02, 0.02, P) * z, rng.uniform(-0.02, 0.02, P) * z, z], 1).astype(np.float32)
        sc["opacities"] = rng.uniform(0.002, 0.05, P).astype(np.float32)
        w2c = np.eye(4, dtype=np.float32)
    elif case == "ties":
        W, H, P = 96, 96, 3000
        sc = random_scene(1000, 3, scale=0.08)
        sc = {k: np.concatenate([v, v, v]) for k, v in sc.items()}
        w2c = np.eye(4, dtype=np.float32)
    elif case == "opaque":
        W, H, P = 128, 128, 8000
        sc = random_scene(P, 4, scale=0.15, opacity_mean=6.0)
        w2c = np.eye(4, dtype=np.float32)
    else:
        raise ValueError(case)
    return W, H, sc, w2c


def _poses(case):
    """the family's own pose, the identity, yaw = 0.9, yaw = pi (turned around), one translated pose"""
    own = _scene(case)[3]
    return np.stack([own, np.eye(4, dtype=np.float32), _pose(0.9), _pose(np.pi), _pose(0.0, (0.15, 0.1, 0.5))]).astype(np.float32)


def _scorer(gpu, W, H, sc, **kw):
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    cam = setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)._replace(bg=torch.from_numpy(BG).to(gpu))
    t = [torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")]
    return FisherScorer(cam, *t, **kw)


def _oracle_view(oracle, W, H, sc, w2c, colours=None):
    """the oracle's single-view forward of the camera-frame means under an identity-view camera: (colour image, (z, 1, z z) image)"""
    cam = oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4))._replace(bg=BG)
    m = oracle.transform_points(w2c, sc["means3D"])
    geo = dict(scales=sc["scales"], rotations=sc["rotations"])
    rgb = oracle.rasterize_forward(cam, m, sc["opacities"], colors_precomp=sc["colors"] if colours is None else colours, **geo)
    z = m[:, 2].astype(np.float32)
    ds = oracle.rasterize_forward(cam, m, sc["opacities"], colors_precomp=np.stack([z, np.ones_like(z), z * z], 1), **geo)
    return rgb, ds


def _same_view(got, v, rgb, ds, what):
    """view v of a render_views result against the oracle's two forwards, bit for bit"""
    assert np.array_equal(bits(got["render"][v]), bits(rgb["color"])), (what, "render")
    assert np.array_equal(bits(got["median_depth"][v]), bits(rgb["depth"])), (what, "median depth")
    assert np.array_equal(bits(got["final_T"][v]), bits(rgb["final_T"])), (what, "final_T")
    assert np.array_equal(bits(got["depth_sil"][v]), bits(ds["color"])), (what, "depth_sil")
    assert int(got["vis_count"][v]) == int((rgb["radii"] > 0).sum()), (what, "vis_count")
    assert int(got["num_rendered"][v]) == int(rgb["num_rendered"]), (what, "num_rendered")


def _same_images(a, b, what, names=IMAGES, va=slice(None), vb=slice(None)):
    for k in names:
        assert np.array_equal(bits(a[k][va]), bits(b[k][vb])), (what, k)


@pytest.fixture(scope="module")
def family(gpu, oracle):
    cache = {}

    def get(case):
        if case not in cache:
            W, H, sc, _ = _scene(case)
            w2cs = _poses(case)
            got = _scorer(gpu, W, H, sc).render_views(torch.from_numpy(w2cs).to(gpu))
            torch.cuda.synchronize()
            cache[case] = (W, H, sc, w2cs, {k: v.cpu().numpy() for k, v in got.items()})
        return cache[case]
    return get


# ---- 1. against the oracle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_five_views_equal_the_oracle_bit_for_bit(family, oracle, case):
    W, H, sc, w2cs, got = family(case)
    assert got["render"].shape == (5, 3, H, W) and got["depth_sil"].shape == (5, 3, H, W)
    assert got["median_depth"].shape == (5, 1, H, W) and got["final_T"].shape == (5, H, W)
    n_vis = []
    for v, w in enumerate(w2cs):
        rgb, ds = _oracle_view(oracle, W, H, sc, w)
        _same_view(got, v, rgb, ds, f"{case} view {v}")
        n_vis.append(int((rgb["radii"] > 0).sum()))
        if n_vis[-1] == 0:
            # a view that sees nothing: the background on all six channels, the default depth, T = 1
            for k in ("render", "depth_sil"):
                assert np.array_equal(bits(got[k][v]), bits(np.broadcast_to(BG[:, None, None], (3, H, W)))), (case, v, k)
            assert (got["median_depth"][v] == 15.0).all() and (got["final_T"][v] == 1.0).all()
    print(f"[render {case}] visible per view {n_vis}, tile instances {got['num_rendered'].tolist()}")
    assert n_vis[0] > 0, n_vis                                        # the family's own view sees the scene
    if case == "ragged":
        assert n_vis[3] == 0 and n_vis[2] == 3102                      # turned around: nothing; yaw 0.9: part of the scene
        empty = float((got["final_T"][2] == 1.0).mean())
        assert 0.3 < empty < 0.45                                      # both empty and covered pixels in one view


# ---- 2. against the single-view GPU API, and at the timed size -------------------------------------------------------------
def test_config1_map_equals_the_single_view_rasteriser(gpu, oracle):
    """10k Gaussians, 8 views, 256 x 256 (room_shell seed 1): every view against fr_forward on the camera-frame means."""
    from fisher_rast import synthetic
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    P, V, W, H = 10000, 8, 256, 256
    act = {k: v.numpy() for k, v in synthetic.activate(synthetic.room_shell(P, seed=1)).items()}
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, seed=1)).numpy().astype(np.float32)
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    sc = FisherScorer(cam, *(torch.from_numpy(act[k]).to(gpu) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")))
    got = {k: v.cpu().numpy() for k, v in sc.render_views(torch.from_numpy(w2c).to(gpu)).items()}
    ocam = oracle.setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4))
    geo = dict(scales=act["scales"], rotations=act["rotations"])
    for v in range(V):
        m = oracle.transform_points(w2c[v], act["means3D"])
        one = hip_forward(gpu, ocam, m, act["opacities"], colors_precomp=act["rgb_colors"], **geo)
        z = m[:, 2].astype(np.float32)
        two = hip_forward(gpu, ocam, m, act["opacities"], colors_precomp=np.stack([z, np.ones_like(z), z * z], 1), **geo)
        assert int((one["radii"] > 0).sum()) > 0                    # (every candidate of this seed sees part of the room: 516 at least)
        assert np.array_equal(bits(got["render"][v]), bits(one["color"])), v
        assert np.array_equal(bits(got["median_depth"][v]), bits(one["depth"])), v
        assert np.array_equal(bits(got["final_T"][v]), bits(one["final_T"])), v
        assert np.array_equal(bits(got["depth_sil"][v]), bits(two["color"])), v
        assert int(got["vis_count"][v]) == int((one["radii"] > 0).sum()) and int(got["num_rendered"][v]) == one["num_rendered"]


def test_four_views_of_the_benchmark_map_equal_the_oracle(gpu, oracle):
    """The size the benchmark tool times: 500k Gaussians (room_shell seed 2), 256 x 256; views 0, 21, 42, 63 of the 64 candidates
    (rendered as a batch of 64, which is what is timed) against the oracle."""
    from fisher_rast import synthetic
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    P, W, H = 500_000, 256, 256
    act = {k: v.numpy() for k, v in synthetic.activate(synthetic.room_shell(P, seed=2)).items()}
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(64, seed=2)).numpy().astype(np.float32)
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)._replace(bg=torch.from_numpy(BG).to(gpu))
    s = FisherScorer(cam, *(torch.from_numpy(act[k]).to(gpu) for k in ("means3D", "rgb_colors", "rotations", "opacities", "scales")))
    got = {k: v.cpu().numpy() for k, v in s.render_views(torch.from_numpy(w2c).to(gpu)).items()}
    sc = dict(means3D=act["means3D"], colors=act["rgb_colors"], rotations=act["rotations"], opacities=act["opacities"], scales=act["scales"])
    for v in (0, 21, 42, 63):
        rgb, ds = _oracle_view(oracle, W, H, sc, w2c[v])
        assert int((rgb["radii"] > 0).sum()) > 10_000
        _same_view(got, v, rgb, ds, f"benchmark map view {v}")


# ---- 3. batch independence, repeatability, spatial order ----------------------------------------------------------------------
def test_a_view_does_not_depend_on_its_batch_and_calls_repeat(gpu):
    W, H, sc, _ = _scene("ragged")
    s = _scorer(gpu, W, H, sc)
    rng = np.random.default_rng(9)
    w = np.stack([_pose(rng.uniform(-0.6, 0.6), rng.uniform(-0.3, 0.3, 3)) for _ in range(64)]).astype(np.float32)
    w2c = torch.from_numpy(w).to(gpu)
    a = s.render_views(w2c)
    b = s.render_views(w2c)
    _same_images(a, b, "second identical call")
    assert torch.equal(a["vis_count"], b["vis_count"]) and torch.equal(a["num_rendered"], b["num_rendered"])
    one = s.render_views(w2c[37:38])
    _same_images(one, a, "view 37 alone against view 37 of 64", va=0, vb=37)
    assert int(one["vis_count"][0]) == int(a["vis_count"][37]) > 0
    few = s.render_views(w2c[35:40])                                   # (5 views: the plain tile map, not the XCD deal)
    _same_images(few, a, "views 35..39 against the batch of 64", vb=slice(35, 40))


def test_spatial_order_gives_the_same_bits(gpu):
    """no two Gaussians of `ragged` share a depth in a view (continuous random means), so the layout order decides nothing"""
    W, H, sc, _ = _scene("ragged")
    w2c = torch.from_numpy(_poses("ragged")).to(gpu)
    a = _scorer(gpu, W, H, sc).render_views(w2c)
    s = _scorer(gpu, W, H, sc, spatial_order=True)
    assert s.order is not None
    b = s.render_views(w2c)
    _same_images(a, b, "spatial_order")
    assert torch.equal(a["vis_count"], b["vis_count"]) and torch.equal(a["num_rendered"], b["num_rendered"])


# ---- 4. overflow and regrow ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["key_buffer", "tile_capacity"])
def test_overflow_writes_nothing_and_render_views_regrows(family, gpu, mode):
    W, H, sc, w2cs, want = family("crowded_tile")
    w2c = torch.from_numpy(w2cs).to(gpu)
    if mode == "key_buffer":
        s = _scorer(gpu, W, H, sc, tile_capacity=0)                    # packed lists in a key buffer too small
        s.per_view_capacity = 16
    else:
        s = _scorer(gpu, W, H, sc, tile_capacity=64)                   # a fixed segment shorter than the longest list (> 4096 keys)
    # the launch: outputs pre-filled with a NaN pattern stay as they were, byte for byte
    pattern = 0x7FC0BEEF
    shapes = dict(render=(5, 3, H, W), depth_sil=(5, 3, H, W), median_depth=(5, 1, H, W), final_T=(5, H, W))
    out = {k: torch.full(shp, pattern, dtype=torch.int32, device=gpu).view(torch.float32) for k, shp in shapes.items()}
    r = s.render_launch(w2c, out=out)
    st = r["status"].cpu().numpy()
    assert st[1] == 1 and (st[3] == 1) == (mode == "tile_capacity"), st
    if mode == "tile_capacity":
        assert st[2] > 4096
    for k in IMAGES:
        assert r[k] is out[k] and bool((out[k].view(torch.int32) == pattern).all()), k
    # ... and render_views grows the buffer and redoes the chunk: the bits of the scorer that never overflowed
    got = s.render_views(w2c)
    _same_images(got, want, f"regrown after {mode} overflow")
    assert np.array_equal(got["vis_count"].cpu().numpy(), want["vis_count"]) and np.array_equal(got["num_rendered"].cpu().numpy(), want["num_rendered"])
    assert (s.tile_capacity == 0 or s.tile_capacity > 4096) and s.per_view_capacity > 16


# ---- 5. chunking --------------------------------------------------------------------------------------------------------------
def test_more_views_than_one_launch_holds(family, gpu, monkeypatch):
    from fisher_rast.ops import FisherScorer
    W, H, sc, w2cs, want = family("opaque")
    s = _scorer(gpu, W, H, sc)
    w2c = torch.from_numpy(np.concatenate([w2cs, w2cs[::-1]])).to(gpu)        # 10 views
    monkeypatch.setattr(FisherScorer, "max_views_per_launch", lambda self: 3)
    launches = []
    real = FisherScorer.render_launch
    monkeypatch.setattr(FisherScorer, "render_launch", lambda self, w, *a, **k: (launches.append(int(w.shape[0])), real(self, w, *a, **k))[1])
    got = s.render_views(w2c)
    assert launches == [3, 3, 3, 1]
    monkeypatch.undo()
    whole = s.render_views(w2c)                                               # one launch
    _same_images(got, whole, "chunks of 3 against one launch")
    parts = [s.render_views(w2c[a:b]) for a, b in ((0, 4), (4, 10))]
    for k in IMAGES + ("vis_count", "num_rendered"):
        assert torch.equal(got[k], torch.cat([p[k] for p in parts])), k
    _same_images(got, want, "first five views against test 1", va=slice(0, 5))
    assert got["render"].shape[0] == 10


# ---- 6. optional outputs, poses_are_c2w ---------------------------------------------------------------------------------------
def test_any_subset_of_outputs_and_both_channel_counts(family, gpu):
    W, H, sc, w2cs, want = family("general")
    s = _scorer(gpu, W, H, sc)
    w2c = torch.from_numpy(w2cs).to(gpu)
    flags = ("render", "features", "depth", "final_T")
    key = dict(render="render", features="depth_sil", depth="median_depth", final_T="final_T")
    for mask in range(1, 16):
        on = {f: bool(mask >> i & 1) for i, f in enumerate(flags)}
        r = s.render_launch(w2c, **on)
        assert int(r["status"].cpu()[1]) == 0
        for f in flags:
            if on[f]:
                assert np.array_equal(bits(r[key[f]]), bits(want[key[f]])), (mask, f)      # (3 and 6 channels agree on `render`)
            else:
                assert r[key[f]] is None
        assert np.array_equal(r["vis_count"].cpu().numpy(), want["vis_count"])
    with pytest.raises(ValueError):
        s.render_launch(w2c, render=False, features=False, depth=False, final_T=False)
    r = s.render_views(w2c, features=False, depth=False, final_T=False)
    assert r["depth_sil"] is None and r["median_depth"] is None and r["final_T"] is None
    assert np.array_equal(bits(r["render"]), bits(want["render"]))


def test_poses_are_c2w_uses_the_librarys_inverse(gpu):
    """c2w with poses_are_c2w=True == poses_are_c2w=False with the matrices the library's inverse kernel makes of them: the adjugate by
    cofactor expansion in double times 1 / det, rounded once to float (`_cofactor_inverse` restates it statement by statement)"""
    W, H, sc, _ = _scene("ragged")
    s = _scorer(gpu, W, H, sc)
    w2cs = _poses("ragged")
    c2w = torch.from_numpy(np.linalg.inv(w2cs.astype(np.float64)).astype(np.float32)).to(gpu)
    a = s.render_views(c2w, poses_are_c2w=True)
    inv = np.stack([_cofactor_inverse(m) for m in c2w.cpu().numpy()])
    b = s.render_views(torch.from_numpy(inv).to(gpu), poses_are_c2w=False)
    _same_images(a, b, "poses_are_c2w")
    assert torch.equal(a["vis_count"], b["vis_count"]) and int(a["vis_count"][0]) > 0
    assert not np.array_equal(inv, w2cs)                      # (the inverse of the inverse is not the matrix it came from, bit for bit)


def _cofactor_inverse(m32):
    """k_invert_poses: the adjugate by cofactor expansion in double, times 1 / det, rounded once to float.
    (The same text as FisherScorer._invert_poses: comparing the two only guards against one of them being edited.  The check that
    is independent of this text is test_poses_are_c2w_uses_the_librarys_inverse, which goes through the kernel itself.)"""
    m = m32.astype(np.float64).reshape(16)
    inv = np.empty(16)
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10]
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10]
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9]
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9]
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10]
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10]
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9]
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9]
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6]
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6]
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5]
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5]
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6]
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6]
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5]
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5]
    det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12]
    return (inv * (1.0 / det)).astype(np.float32).reshape(4, 4)


# ---- 7. the Python surface ----------------------------------------------------------------------------------------------------
def test_render_at_poses_equals_the_forward_pair_route_per_pose(gpu):
    from models.SLAM.gaussian import GaussianSLAM
    from models.SLAM.gaussian_object import GaussianObjectSLAM
    from models.SLAM.utils.slam_helpers import render_rgb_depth_sil
    W, H, sc, _ = _scene("ragged")
    raw = dict(means3D=sc["means3D"], rgb_colors=sc["colors"], unnorm_rotations=sc["rotations"] * 2.0,
               logit_opacities=np.log(sc["opacities"] / (1 - sc["opacities"])).reshape(-1, 1), log_scales=np.log(sc["scales"]))
    params = {k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in raw.items()}
    slam = GaussianSLAM(params=params, intrinsics=np.asarray(intrinsics(W, H)), width=W, height=H, device=gpu)
    w2cs = _poses("ragged")
    c2ws = np.linalg.inv(w2cs.astype(np.float64)).astype(np.float32)
    got = slam.render_at_poses(c2ws)
    assert set(got) == {"render", "depth", "silhouette"}
    assert got["render"].shape == (5, 3, H, W) and got["depth"].shape == (5, 1, H, W) and got["silhouette"].shape == (5, 1, H, W)
    lst = slam.render_at_poses([torch.from_numpy(c).to(gpu) for c in c2ws])       # a list of device tensors, as pose_eval takes them
    for k in got:
        assert torch.equal(got[k], lst[k]), k
    x, y, z = (slam.params["means3D"][:, k] for k in range(3))
    eye = torch.eye(4, device=gpu)
    for v, c in enumerate(c2ws):
        w = torch.from_numpy(_cofactor_inverse(c)).to(gpu)                         # what the library makes of the pose
        # the fixed-order camera-frame means, every product and sum rounded on its own
        m = torch.stack([((x * w[r, 0] + y * w[r, 1]) + z * w[r, 2]) + w[r, 3] for r in range(3)], dim=1)
        im, radius, depth_sil, _ = render_rgb_depth_sil(slam.params, slam.cam, eye, m)
        assert np.array_equal(bits(got["render"][v]), bits(im)), v
        assert np.array_equal(bits(got["depth"][v]), bits(depth_sil[0:1])), v
        assert np.array_equal(bits(got["silhouette"][v]), bits(depth_sil[1:2])), v
    assert float(got["silhouette"][0].max()) > 0.5 and float(got["silhouette"][3].max()) == 0.0        # (bg = 0: the turned view shows nothing)
    full = slam.render_views(w2cs)                                                 # world->camera poses, every output
    assert full["final_T"].shape == (5, H, W) and int(full["vis_count"][3]) == 0 and int(full["vis_count"][0]) > 0
    assert torch.equal(full["depth_sil"][3, 1], 1.0 - full["final_T"][3])         # (nothing composited: silhouette 0, T 1)
    # the object class inherits the same methods
    obj = GaussianObjectSLAM(params=params, intrinsics=np.asarray(intrinsics(W, H)), width=W, height=H, device=gpu)
    assert torch.equal(obj.render_at_poses(c2ws)["render"], got["render"])


def test_images_beyond_4096_tiles_loop_over_the_single_view_rasteriser(gpu, oracle):
    """1040 x 1024 = 4160 tiles: the batched entry point rejects the size; render_views loops, with the same fixed-order means"""
    W, H = 16 * 65, 16 * 64
    sc = random_scene(400, 6, scale=0.05)
    s = _scorer(gpu, W, H, sc)
    assert s.tiles == 4160
    w2cs = np.stack([np.eye(4, dtype=np.float32), _pose(0.3)])
    got = {k: v.cpu().numpy() for k, v in s.render_views(torch.from_numpy(w2cs).to(gpu)).items()}
    for v, w in enumerate(w2cs):
        rgb, ds = _oracle_view(oracle, W, H, sc, w)
        _same_view(got, v, rgb, ds, f"large image view {v}")
    # camera-to-world poses: inverted as the library's kernel inverts them
    c2w = np.linalg.inv(w2cs.astype(np.float64)).astype(np.float32)
    inv = s._invert_poses(torch.from_numpy(c2w).to(gpu)).cpu().numpy()
    assert np.array_equal(bits(inv), bits(np.stack([_cofactor_inverse(m) for m in c2w])))
    a = s.render_views(torch.from_numpy(c2w[1:2]).to(gpu), poses_are_c2w=True)
    b = s.render_views(torch.from_numpy(inv[1:2]).to(gpu))
    _same_images(a, b, "large image, poses_are_c2w")
