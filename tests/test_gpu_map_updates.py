"""-m gpu: a FisherScorer holds the caller's map tensors (no copies) and lives across map updates -- optimiser steps, densification,
`replicate_map` refills.  Since the static records (means, cov3D, colours, shared H_inv rows) are reused between calls
(fr_fisher_cfg.reuse_static), a scorer whose map was changed IN PLACE must pack them again: after the change, every mode must give
what a fresh scorer built on the changed map gives (scores and pose matrices bit for bit, diagonals to the order of their float
atomics), and what the oracle gives.  Every cell also checks that the change moves its result by far more than the tolerance.

Modes that reuse the static records are the compact-record ones of fr_fisher_views: scores (shared or per-view H_inv), out_H (shared
or per view, 4 or 11 columns) and out_H under a per-view upstream-gradient image.  Controls that pack on every call: scores and out_H
in one call (the two-pass fall-back) and the pose Fisher (fr_fisher_pose_views).  Opacities are read live by every mode."""
import numpy as np
import pytest
import torch

from scenes import intrinsics, random_scene, rel_err

pytestmark = pytest.mark.gpu

P, W, H, V = 8000, 112, 80, 6
NAMES = ("means3D", "rgb_colors", "rotations", "opacities", "scales")
ATTR = dict(means3D="means3D", rgb_colors="colors", rotations="rotations", opacities="opacities", scales="scales")
REUSING = ("score", "score_pv", "outh", "outh_pv", "image")
CONTROLS = ("both", "pose")


@pytest.fixture(scope="module")
def scene(gpu, oracle):
    from fisher_rast import synthetic
    from models.SLAM.utils.recon_helpers import setup_camera
    act = synthetic.activate(synthetic.room_shell(P, seed=70))
    # anisotropic splats, so that a turned quaternion changes the covariance by more than rounding
    act["scales"] = (act["scales"] * torch.tensor([3.0, 1.0, 0.4])).contiguous()
    act = {k: v.contiguous() for k, v in act.items()}
    K = synthetic.intrinsics(W, H)
    cam = setup_camera(W, H, K, np.eye(4), device=gpu)
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(V, seed=71))
    g = torch.Generator().manual_seed(72)
    # on the device once: a call reuses the static records only for the very same shared H_inv TENSOR
    hinv = {c: (torch.rand((P, c), generator=g) * 2 + 0.05).to(gpu) for c in (4, 11)}
    hinv_pv = {c: (torch.rand((V, P, c), generator=g) + 0.05).to(gpu) for c in (4, 11)}
    img = (torch.randn((V, 3, H, W), generator=g) * 1e-3).to(gpu)
    return dict(act=act, cam=cam, ocam=oracle.setup_camera(W, H, K, np.eye(4)), w2c=w2c, hinv=hinv, hinv_pv=hinv_pv, img=img)


def _map(scene, gpu):
    """the caller's tensors: a private copy of the scene on the device, fp32 contiguous (what FisherScorer holds without copying)"""
    return {k: scene["act"][k].to(gpu).clone() for k in NAMES}


def _scorer(scene, tensors, columns, **kw):
    from fisher_rast.ops import FisherScorer
    return FisherScorer(scene["cam"], *(tensors[k] for k in NAMES), columns=columns, **kw)


def _call(sc, scene, mode, gpu):
    """one call of `mode`: {"scores", "H", "pose"} (None where the mode has no such output), on the host"""
    C, w = sc.columns, scene["w2c"].to(gpu)
    out = dict(scores=None, H=None, pose=None)
    if mode == "pose":
        out["pose"] = sc.pose_fisher(w).cpu()
        return out
    kw = {}
    if mode in ("score", "both"):
        kw = dict(H_inv=scene["hinv"][C]) if mode == "score" else dict(H_inv=scene["hinv_pv"][C], H_inv_per_view=True)
    elif mode == "score_pv":
        kw = dict(H_inv=scene["hinv_pv"][C], H_inv_per_view=True)
    if mode == "outh":
        kw["out_H"] = torch.zeros((P, C), device=gpu)
    elif mode in ("outh_pv", "image", "both"):
        kw.update(out_H=torch.zeros((V, P, C), device=gpu), out_H_per_view=True)
    if mode == "image":
        kw["dL_image"] = scene["img"]
    r = sc.run(w, **kw)
    out["scores"] = None if r["scores"] is None else r["scores"].cpu()
    out["H"] = None if "out_H" not in kw else kw["out_H"].cpu()
    return out


def _same(a, b, mode, what):
    """scores and pose matrices bit for bit (the two-pass kernel sums its scores with atomics), diagonals to atomics order"""
    if a["scores"] is not None:
        if mode == "both":
            assert rel_err(a["scores"].numpy(), b["scores"].numpy()) < 1e-5, (what, a["scores"], b["scores"])
        else:
            assert torch.equal(a["scores"], b["scores"]), (what, a["scores"], b["scores"])
        assert float(b["scores"].min()) > 0, what
    if a["H"] is not None:
        assert float(b["H"].abs().max()) > 0 and rel_err(a["H"].numpy(), b["H"].numpy()) < 1e-5, (what, rel_err(a["H"].numpy(), b["H"].numpy()))
    if a["pose"] is not None:
        assert torch.equal(a["pose"], b["pose"]), what


def _moved(after, before, what, by=1e-3):
    """the change is visible: every output moves by far more than the tolerances of `_same`"""
    for k in ("scores", "H", "pose"):
        if after[k] is not None:
            d = rel_err(after[k].numpy(), before[k].numpy())
            assert d > by, (what, k, d)


def _change(t, name):
    """an in-place tensor op on every second Gaussian (the version counter moves)"""
    if name == "means3D":
        t[::2] += torch.tensor([0.1, -0.05, 0.08], device=t.device)
    elif name == "rgb_colors":
        t[::2].neg_().add_(1.0)
    elif name == "rotations":
        t[::2] = t[::2].roll(1, dims=1)                     # another unit quaternion
    elif name == "scales":
        t[::2] *= 1.5
    elif name == "opacities":
        t[::2] *= 0.5


def _oracle_check(sc, scene, mode, got, oracle):
    """the changed scorer against the oracle on the changed map, at the parity tests' tolerance"""
    C = sc.columns
    m = {k: getattr(sc, ATTR[k]).cpu().numpy() for k in NAMES}
    args = (m["means3D"], m["rgb_colors"], m["rotations"], m["opacities"].reshape(-1, 1), m["scales"])
    rows = []
    for v, w in enumerate(scene["w2c"].numpy()):
        cur, _, fwd, _ = oracle.compute_hessian(scene["ocam"], w, *args, columns=C, return_all=True)
        if mode == "image":
            g = oracle.rasterize_backward(scene["ocam"], fwd, scene["img"][v].cpu().numpy(), power=2)
            parts = [g["dL_dmeans3D"], g["dL_dopacity"]] + ([g["dL_dscales"], g["dL_drotations"]] if C == 11 else [])
            cur = np.concatenate(parts, axis=1)
        rows.append(cur.astype(np.float64))
    rows = np.stack(rows)
    if mode in ("score", "score_pv", "both"):
        hi = scene["hinv"][C].cpu().numpy()[None] if mode == "score" else scene["hinv_pv"][C].cpu().numpy()
        want = (rows * hi.astype(np.float64)).sum(axis=(1, 2))
        assert rel_err(got["scores"].numpy(), want) < 1e-4, (mode, got["scores"], want)
    if mode == "outh":
        assert rel_err(got["H"].numpy(), rows.sum(axis=0)) < 1e-4, mode
    elif mode in ("outh_pv", "image", "both"):
        assert rel_err(got["H"].numpy(), rows) < 1e-4, mode


CELLS = [("scorer", -1), ("caller", -1), ("scorer", 0)]


@pytest.mark.parametrize("via,tile_capacity", CELLS, ids=["scorer", "caller", "scorer-packed"])
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("mode", REUSING + CONTROLS)
def test_in_place_map_change_equals_a_fresh_scorer(scene, gpu, oracle, mode, columns, name, via, tile_capacity):
    mine = _map(scene, gpu)
    sc = _scorer(scene, mine, columns, tile_capacity=tile_capacity)
    assert (sc.tile_capacity == 0) == (tile_capacity == 0)
    a = _call(sc, scene, mode, gpu)
    key = sc._static_key
    b = _call(sc, scene, mode, gpu)
    if mode in REUSING:
        # an unchanged map keeps its key: the second call was launched with reuse_static set, and gives the same numbers
        assert key is not None and sc._static_key == key
        assert sc._static_hinv is (scene["hinv"][columns] if mode == "score" else None)
    elif mode == "both":
        assert sc._static_key is None
    _same(a, b, mode, "repeat")
    held = getattr(sc, ATTR[name])
    with torch.no_grad():
        _change(held if via == "scorer" else mine[name], name)
    # the scorer holds the caller's storage: the change shows through both names
    assert torch.equal(held.reshape(-1), mine[name].reshape(-1))
    c = _call(sc, scene, mode, gpu)
    fresh = _call(_scorer(scene, {k: v.clone() for k, v in mine.items()}, columns, tile_capacity=tile_capacity), scene, mode, gpu)
    _same(c, fresh, mode, (mode, name, via))
    _moved(c, a, (mode, name, via))
    if name == "means3D" and via == "scorer" and tile_capacity < 0 and mode != "pose":
        _oracle_check(sc, scene, mode, c, oracle)          # the scorer and the fresh scorer are not both wrong (once per mode)


def test_pose_fisher_after_an_in_place_change_matches_the_oracle(gpu, oracle):
    """the pose mode's oracle check, on a scene small enough for the per-pixel reference of tests/pose_fisher_ref.py"""
    import pose_fisher_ref as pf
    from test_gpu_pose_fisher import K_POSE
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    w, h = 64, 48
    s = random_scene(300, 1, zmin=1.0, spread=0.8)
    t = {k: torch.from_numpy(np.ascontiguousarray(s[k])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")}
    cam = setup_camera(w, h, intrinsics(w, h), np.eye(4), device=gpu)
    sc = FisherScorer(cam, *(t[k] for k in ("means3D", "colors", "rotations", "opacities", "scales")))
    w2c = np.eye(4, dtype=np.float32)[None]
    before = sc.pose_fisher(torch.from_numpy(w2c).to(gpu)).cpu().numpy()
    with torch.no_grad():
        t["means3D"][::2] += torch.tensor([0.05, -0.03, 0.1], device=gpu)
    got = sc.pose_fisher(torch.from_numpy(w2c).to(gpu)).cpu().numpy()[0].astype(np.float64)
    s["means3D"] = t["means3D"].cpu().numpy()
    H64, JJ, _ = pf.pose_hessian_ref(oracle.setup_camera(w, h, intrinsics(w, h), np.eye(4)), w2c[0], s)
    tol = 1e-4 * np.abs(H64) + K_POSE * 2.0 ** -24 * JJ
    assert (np.abs(got - H64) <= tol).all(), (pf.k_needed(got, H64, JJ), got, H64)
    assert rel_err(got, before[0]) > 1e-3


@pytest.mark.parametrize("mode", ["score", "outh_pv", "pose"])
def test_writes_behind_the_version_counter_need_map_changed(scene, gpu, mode):
    """`.data` (like a collective, DLPack or a raw pointer) writes without bumping the version: `map_changed()` tells the scorer.
    (What a scorer computes without it is undefined and not asserted.)"""
    mine = _map(scene, gpu)
    sc = _scorer(scene, mine, 4)
    a = _call(sc, scene, mode, gpu)
    _call(sc, scene, mode, gpu)
    v = sc.means3D._version
    sc.means3D.data[::2] += torch.tensor([0.1, -0.05, 0.08], device=gpu)
    assert sc.means3D._version == v
    sc.map_changed()
    assert sc._static_key is None
    c = _call(sc, scene, mode, gpu)
    fresh = _call(_scorer(scene, {k: t.clone() for k, t in mine.items()}, 4), scene, mode, gpu)
    _same(c, fresh, mode, mode)
    _moved(c, a, mode)


@pytest.mark.parametrize("how", ["in_place", "map_changed"])
def test_spatial_order_follows_the_means(scene, gpu, how):
    """spatial_order=True: the Z-curve order is taken again when the means have moved (in place through a tensor op, or behind the
    version counter followed by map_changed), so the scorer equals a fresh spatial-order scorer on the moved map"""
    from fisher_rast.ops import spatial_order_of
    mine = _map(scene, gpu)
    sc = _scorer(scene, mine, 4, spatial_order=True)
    a = _call(sc, scene, "score", gpu)
    _call(sc, scene, "score", gpu)
    old = sc.order.clone()
    g = torch.Generator().manual_seed(5)
    step = (torch.rand((P, 3), generator=g) * 2 - 1).to(gpu) * torch.tensor([2.0, 0.5, 2.0], device=gpu)
    if how == "in_place":
        with torch.no_grad():
            sc.means3D[::3] += step[::3]
    else:
        sc.means3D.data[::3] += step[::3]
        sc.map_changed()
    c = _call(sc, scene, "score", gpu)
    want = spatial_order_of(mine["means3D"])
    assert torch.equal(sc.order, want) and not torch.equal(want, old)
    fresh = _scorer(scene, {k: t.clone() for k, t in mine.items()}, 4, spatial_order=True)
    _same(c, _call(fresh, scene, "score", gpu), "score", how)
    _moved(c, a, how)
    _same(_call(sc, scene, "pose", gpu), _call(fresh, scene, "pose", gpu), "pose", how)


def test_unchanged_map_keeps_the_static_key(scene, gpu):
    """the benchmark's loop (one shared H_inv, the same views, the map untouched): the key stays put call after call, so every call
    after the first is launched with reuse_static set"""
    mine = _map(scene, gpu)
    sc = _scorer(scene, mine, 4)
    w, hi = scene["w2c"].to(gpu), scene["hinv"][4]
    first = sc.run(w, H_inv=hi)["scores"]
    key = sc._static_key
    assert key is not None
    for _ in range(5):
        r = sc.launch(w, H_inv=hi)
        assert sc._static_key == key
    assert torch.equal(r["scores"], first)


# ---- the SLAM surfaces ------------------------------------------------------------------------------------------------------------

def _slam_scene():
    from fisher_rast import synthetic
    params = synthetic.room_shell(P, seed=80)
    K = synthetic.intrinsics(W, H)
    c2w = synthetic.candidate_poses(4, seed=81)
    kf_w2c = synthetic.invert_rigid(synthetic.candidate_poses(2, seed=82))
    g = torch.Generator().manual_seed(83)
    Nr = 600
    rg = dict(means3D=(torch.rand((Nr, 3), generator=g) - 0.5) * torch.tensor([8.0, 2.0, 8.0]),
              rotations=torch.nn.functional.normalize(torch.randn((Nr, 4), generator=g)),
              opacity=torch.rand((Nr, 1), generator=g) * 0.8 + 0.1,
              scales=torch.rand((Nr, 3), generator=g) * 0.05 + 0.01)
    return params, K, c2w, kf_w2c, rg


def _slam(cls, params, K, kf_w2c, gpu):
    slam = cls(params=params, intrinsics=K, width=W, height=H, device=gpu)
    for w in kf_w2c:
        slam.add_keyframe(w.clone())
    return slam


def _surfaces(slam, c2w, rg):
    poses = [p for p in c2w.to(slam._device())]
    w2c = torch.linalg.inv(c2w[0].double()).float()
    return dict(hess=slam.compute_Hessian(w2c, return_points=True, random_gaussian_params=rg).cpu(),
                h_train=slam.compute_H_train(rg).cpu(),
                pose_eval=slam.pose_eval(poses, random_gaussian_params=rg)[0].cpu(),
                pose_H=slam.pose_Hessians(torch.linalg.inv(c2w.double()).float()).cpu())


@pytest.mark.parametrize("update", ["adam", "prune", "data"])
@pytest.mark.parametrize("cls_name", ["GaussianSLAM", "GaussianObjectSLAM"])
def test_slam_surfaces_follow_map_updates(gpu, cls_name, update):
    """(a) an optimiser step on slam.params (in place), (b) a prune that replaces the tensors, (c) a `.data` write followed by
    increment_version (what replicate_map does): compute_Hessian, compute_H_train, pose_eval and pose_Hessians then equal a fresh
    SLAM object's on clones of the updated params"""
    import models.gaussian_slam as mgs
    from models.SLAM.utils.slam_external import prune_mask
    cls = getattr(mgs, cls_name)
    params, K, c2w, kf_w2c, rg = _slam_scene()
    rg = rg if cls_name == "GaussianObjectSLAM" else None
    slam = _slam(cls, {k: v.clone() for k, v in params.items()}, K, kf_w2c, gpu)
    if update == "adam":
        slam.params = {k: torch.nn.Parameter(v) for k, v in slam.params.items()}
    before = _surfaces(slam, c2w, rg)
    again = _surfaces(slam, c2w, rg)                        # the caches are warm: scorer, static records, 1 / (H_train + reg)
    assert torch.equal(again["pose_H"], before["pose_H"]) and torch.equal(again["pose_eval"], before["pose_eval"])
    if update == "adam":
        opt = torch.optim.Adam(list(slam.params.values()), lr=0.02)
        g = torch.Generator().manual_seed(84)
        loss = sum((v * torch.randn(v.shape, generator=g).to(gpu)).sum() for v in slam.params.values())
        opt.zero_grad()
        loss.backward()
        opt.step()
    elif update == "prune":
        keep = ~prune_mask(slam.params, 0.3)
        assert 0 < int((~keep).sum()) < P // 2
        slam.params = {k: v[keep].contiguous() for k, v in slam.params.items()}
    else:
        for k, d in (("means3D", torch.tensor([0.1, -0.05, 0.08], device=gpu)), ("log_scales", 0.3)):
            slam.params[k].data[::2] += d
            torch.autograd.graph.increment_version(slam.params[k])
    after = _surfaces(slam, c2w, rg)
    fresh = _surfaces(_slam(cls, {k: v.detach().clone() for k, v in slam.params.items()}, K, kf_w2c, gpu), c2w, rg)
    assert torch.equal(after["pose_H"], fresh["pose_H"])
    for k in ("hess", "h_train"):
        assert after[k].shape == fresh[k].shape and rel_err(after[k].numpy(), fresh[k].numpy()) < 1e-5, k
    assert torch.allclose(after["pose_eval"], fresh["pose_eval"], rtol=1e-5)
    # the update is visible in every output
    for k in ("pose_H", "pose_eval"):
        assert rel_err(after[k].numpy(), before[k].numpy()) > 1e-3, k
    for k in ("hess", "h_train"):
        assert after[k].shape != before[k].shape or rel_err(after[k].numpy(), before[k].numpy()) > 1e-3, k
