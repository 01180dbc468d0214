"""-m gpu: the camera-pose Fisher information (fr_fisher_pose_views / FisherScorer.pose_fisher) against the oracle-built reference of
tests/pose_fisher_ref.py (one-hot backward in the arbiter build -> g_{p,i} -> j_p -> sum_p j_p j_p^T), on several scene families;
symmetry and semi-definiteness; determinism (two calls, one view alone against the same view in a 64-view batch); overflow; the 4- and
11-column scorers; the SLAM surface; and the path evaluator's pose term against a serial loop of the reference.

Tolerance per entry:  |H - H64|_ab <= 1e-4 |H64_ab| + K 2^-24 sum_p J+_{p,a} J+_{p,b},  J+_p = sum_i |[g_{p,i}; m_i x g_{p,i}]|: a pixel's
j_p is a signed sum, so its rounding is a multiple of eps times the size of the terms it sums, not of the sum."""
import numpy as np
import pytest
import torch

import pose_fisher_ref as pf
from scenes import random_scene, intrinsics

pytestmark = pytest.mark.gpu

# multiple of 2^-24 sum_p J+_a J+_b allowed (the need is printed per family)
K_POSE = 16.0


def _yaw(k, base=None):
    yaw, t = 0.06 * k, np.array([0.04 * k, -0.02 * k, 0.03 * k], np.float32)
    c, s = np.cos(yaw), np.sin(yaw)
    d = np.eye(4, dtype=np.float32)
    d[:3, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)
    d[:3, 3] = t
    return (d @ (np.eye(4, dtype=np.float32) if base is None else base)).astype(np.float32)


def _family(case):
    """(W, H, scene in world coordinates, [V,4,4] w2c)"""
    rng = np.random.default_rng({"random": 1, "border": 11, "dense": 2, "giant": 3}[case])
    if case == "random":
        W, H = 64, 48
        sc = random_scene(300, 1, zmin=1.0, spread=0.8)
    elif case == "border":                        # splats around the frustum's edges: clamped txtz (limx / limy) and partial tiles
        W, H, P = 64, 48, 300
        z = rng.uniform(0.8, 5.0, P)
        band = rng.uniform(0.9, 1.8, P) * rng.choice([-1.0, 1.0], P)
        free = rng.uniform(-1.4, 1.4, P)
        side = rng.random(P) < 0.5
        sc = random_scene(P, 11, scale=0.08)
        sc["means3D"] = np.stack([np.where(side, band, free) * z, np.where(side, free, band) * z, z], 1).astype(np.float32)
    elif case == "dense":                         # hundreds of faint splats on a few tiles: deep lists, T far from its cut-off
        W, H, P = 48, 32, 500
        sc = random_scene(P, 2, scale=0.03)
        z = rng.uniform(1.5, 5.0, P)
        sc["means3D"] = np.stack([rng.uniform(-0.15, 0.15, P) * z, rng.uniform(-0.15, 0.15, P) * z, z], 1).astype(np.float32)
        sc["opacities"] = rng.uniform(0.02, 0.3, P).astype(np.float32)
    elif case == "giant":                         # near-plane giants in front of an ordinary scene: every pixel sees them
        W, H = 48, 32
        sc = random_scene(200, 3, zmin=1.5, spread=0.7)
        g = dict(means3D=np.array([[0.01, 0.02, 0.05], [-0.1, 0.05, 0.2], [0.2, -0.1, 0.4]], np.float32),
                 scales=np.array([[0.3, 0.2, 0.05], [0.5, 0.5, 0.1], [0.8, 0.3, 0.3]], np.float32),
                 rotations=np.array([[1, 0, 0, 0], [0.9, 0.1, 0.3, 0.2], [0.7, -0.2, 0.1, 0.6]], np.float32),
                 opacities=np.array([0.05, 0.1, 0.2], np.float32), colors=rng.uniform(0, 1, (3, 3)).astype(np.float32))
        g["rotations"] /= np.linalg.norm(g["rotations"], axis=1, keepdims=True)
        sc = {k: np.concatenate([g[k], sc[k]]).astype(np.float32) for k in sc}
    else:
        raise ValueError(case)
    return W, H, sc, np.stack([_yaw(0), _yaw(1)])


def _scorer(gpu, W, H, sc, columns=4, **kw):
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    cam = setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)
    t = [torch.from_numpy(np.ascontiguousarray(sc[k])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")]
    return FisherScorer(cam, *t, columns=columns, **kw)


def _check(got, H64, JJ, case):
    got = np.asarray(got, np.float64)
    k = pf.k_needed(got, H64, JJ)
    print(f"[pose {case}] K needed {k:.3g} of K_POSE {K_POSE}; |H64| max {np.abs(H64).max():.3e}")
    tol = 1e-4 * np.abs(H64) + K_POSE * 2.0 ** -24 * JJ
    assert (np.abs(got - H64) <= tol).all(), (case, k, got, H64)


@pytest.mark.parametrize("case", ["random", "border", "dense", "giant"])
def test_pose_fisher_matches_oracle_reference(gpu, oracle, case):
    W, H, sc, w2cs = _family(case)
    s = _scorer(gpu, W, H, sc)
    got = s.pose_fisher(torch.from_numpy(w2cs).to(gpu)).cpu().numpy()
    assert got.shape == (len(w2cs), 6, 6) and np.isfinite(got).all()
    ocam = oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4))
    for v, w in enumerate(w2cs):
        H64, JJ, _ = pf.pose_hessian_ref(ocam, w, sc)
        assert np.abs(H64).max() > 0
        _check(got[v], H64, JJ, f"{case} view {v}")
        # symmetric (both triangles are the same numbers) and positive semi-definite up to rounding
        assert np.array_equal(got[v], got[v].T)
        ev = np.linalg.eigvalsh(got[v].astype(np.float64))
        assert ev.min() >= -1e-5 * ev.max(), ev


def test_empty_view_is_exact_zero(gpu):
    W, H, sc, _ = _family("random")
    s = _scorer(gpu, W, H, sc)
    back = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)          # turned around: every Gaussian is behind the camera
    w2c = torch.from_numpy(np.stack([back, _yaw(0)])).to(gpu)
    r = s.pose_launch(w2c)
    got = r["pose_H"].cpu().numpy()
    assert int(r["status"].cpu()[1]) == 0 and int(r["vis_count"].cpu()[0]) == 0
    assert np.array_equal(got[0], np.zeros((6, 6), np.float32)) and np.abs(got[1]).max() > 0


def test_pose_fisher_is_deterministic_and_batch_independent(gpu):
    W, H, sc, _ = _family("random")
    s = _scorer(gpu, W, H, sc)
    w2c = torch.from_numpy(np.stack([_yaw(k % 9, _yaw(k // 9)) for k in range(64)])).to(gpu)
    a = s.pose_fisher(w2c).cpu().numpy()
    b = s.pose_fisher(w2c).cpu().numpy()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for v in (0, 13, 63):
        one = s.pose_fisher(w2c[v:v + 1]).cpu().numpy()
        assert np.array_equal(one[0].view(np.uint32), a[v].view(np.uint32)), v
    # poses_are_c2w: the library inverts them; same views, same numbers up to the inverse's rounding
    c2w = torch.linalg.inv(w2c.double()).float()
    c = s.pose_fisher(c2w, poses_are_c2w=True).cpu().numpy()
    assert np.allclose(c, a, rtol=1e-3, atol=1e-6 * np.abs(a).max())
    # 11 columns: the same kernel, the same bits
    s11 = _scorer(gpu, W, H, sc, columns=11)
    assert np.array_equal(s11.pose_fisher(w2c).cpu().numpy().view(np.uint32), a.view(np.uint32))


def test_overflow_sets_status_and_writes_nothing(gpu):
    W, H, sc, w2cs = _family("dense")
    w2c = torch.from_numpy(w2cs).to(gpu)
    want = _scorer(gpu, W, H, sc).pose_fisher(w2c).cpu().numpy()
    # a fixed key segment shorter than the longest tile list, and packed lists in a key buffer too small
    for kw in (dict(tile_capacity=64), dict(tile_capacity=0)):
        s = _scorer(gpu, W, H, sc, **kw)
        if kw["tile_capacity"] == 0:
            s.per_view_capacity = 16
        out = torch.full((len(w2cs), 6, 6), 7.0, device=gpu)
        r = s.pose_launch(w2c, out=out)
        st = r["status"].cpu().numpy()
        assert st[1] == 1 and (st[3] == 1) == (kw["tile_capacity"] > 0), (kw, st)
        assert (out.cpu().numpy() == 7.0).all()
        # ... and pose_fisher grows the buffer and redoes the batch: the same numbers as a scorer that never overflowed
        assert np.allclose(s.pose_fisher(w2c).cpu().numpy(), want, rtol=1e-5, atol=0.0)


def test_slam_surface(gpu, oracle):
    from models.SLAM.gaussian import GaussianSLAM
    W, H, sc, w2cs = _family("random")
    params = dict(means3D=sc["means3D"], rgb_colors=sc["colors"], unnorm_rotations=sc["rotations"] * 2.0,
                  logit_opacities=np.log(sc["opacities"] / (1 - sc["opacities"])).reshape(-1, 1),
                  log_scales=np.log(sc["scales"]))
    slam = GaussianSLAM(params={k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in params.items()},
                        intrinsics=np.asarray(intrinsics(W, H)), width=W, height=H, device=gpu)
    many = slam.pose_Hessians(w2cs)
    assert many.shape == (2, 6, 6) and many.device.type == "cuda"
    for v in range(2):
        one = slam.compute_pose_Hessian(w2cs[v])
        assert one.shape == (6, 6) and torch.equal(one, many[v])
    # against the reference on the activated map the surface builds (gaussian.py:1529-1533)
    act = dict(sc, rotations=torch.nn.functional.normalize(torch.from_numpy(params["unnorm_rotations"])).numpy(),
               opacities=torch.sigmoid(torch.from_numpy(params["logit_opacities"].astype(np.float32))).numpy().reshape(-1),
               scales=torch.exp(torch.from_numpy(params["log_scales"].astype(np.float32))).numpy())
    H64, JJ, _ = pf.pose_hessian_ref(oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4)), w2cs[1], act)
    _check(many[1].cpu().numpy(), H64, JJ, "slam")
    # the reference's compute_Hessian(return_pose=True) placeholder stays as it is
    cur_H, pose_H = slam.compute_Hessian(w2cs[0], return_pose=True)
    assert torch.equal(pose_H.cpu(), torch.eye(6))


def test_path_pose_term_matches_serial_reference(gpu, oracle):
    from fisher_rast.path_eval import compute_next_campos, evaluate_paths
    W, H = 48, 32
    sc = random_scene(250, 7, zmin=1.5, spread=0.7)
    s = _scorer(gpu, W, H, sc)
    ocam = oracle.setup_camera(W, H, intrinsics(W, H), np.eye(4))
    args = (sc["means3D"], sc["colors"], sc["rotations"], sc["opacities"], sc["scales"])
    kf = np.stack([_yaw(1), _yaw(2)])
    H_train = oracle.compute_h_train(ocam, kf, *args)
    start = np.eye(4)
    rng = np.random.default_rng(4)
    paths = [list(rng.integers(1, 4, size=n)) for n in (3, 2, 4)]
    finals = [0.3, -0.1, 0.2]
    lam, acc, w_point, w_pose, reg = 0.1, 2, 1.0, 0.2, 1e-9
    kw = dict(H_reg_lambda=lam, acc_H_train_every=acc, path_point_weight=w_point, path_pose_weight=w_pose)
    Ht = torch.from_numpy(H_train).to(gpu)
    got = evaluate_paths(s, start, paths, finals, Ht, pose_fisher=True, pose_reg=reg, **kw)
    want = []
    for acts, fin in zip(paths, finals):
        H_path, pose, total = H_train.copy(), start.copy(), 0.0
        for n, a in enumerate(acts, 1):
            pose = compute_next_campos(pose, int(a))
            w2c = np.linalg.inv(pose).astype(np.float32)
            H64, _, _ = pf.pose_hessian_ref(ocam, w2c, sc)
            sign, ld = np.linalg.slogdet(H64 + reg * np.eye(6))
            total += w_pose * (ld if sign > 0 else -np.inf)
            if (n + 1) % acc == 0:
                cur_H, _ = oracle.compute_hessian(ocam, w2c, *args)
                total += w_point * np.log(np.sum(cur_H.astype(np.float64) / (H_path.astype(np.float64) + lam)))
                H_path = H_path + cur_H
        want.append((total + fin) / len(acts))
    print("[pose paths]", got, want)
    assert np.allclose(got, want, rtol=1e-3, atol=1e-4), (got, want)
    # pose_fisher=False: the evaluator as it was
    base = evaluate_paths(s, start, paths, finals, Ht, **kw)
    assert evaluate_paths(s, start, paths, finals, Ht, pose_fisher=False, **kw) == base
    assert not np.allclose(base, got)
