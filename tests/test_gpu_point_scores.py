"""-m gpu: per-Gaussian view scores and their running maximum (fr_fisher_point_views / FisherScorer.point_scores /
PointScoreOps.pose_eval_points) on the adversarial scene families of test_gpu_scorer_adversarial.py, against the oracle's
compute_Hessian contracted with H_inv in binary64:  want[v, i] = sum_c cur_o[v, i, c] H_inv[i, c].
Tolerance: the project's entry rule (1e-4, widened by K_DEV times what the reference's own binary32 chain loses on that Gaussian,
capped) carried through the positive-weighted sum:  tol[v, i] = sum_c tol_entry[v, i, c] H_inv[i, c] + 1e-7 max|want|.
The identities (running maximum, untouched entries, reproducible view scores) are exact."""
import ctypes

import numpy as np
import pytest
import torch

from scenes import intrinsics, rel_err
from test_gpu_rasterizer_parity import CASES
from test_gpu_scorer_adversarial import _family, _views, _entry_tolerance, K_DEV, WIDEN_CAP

pytestmark = pytest.mark.gpu

FAMILIES = CASES + ["thresholds", "border"]


@pytest.fixture(scope="module")
def family(gpu, oracle):
    cache = {}

    def get(case):
        if case not in cache:
            from fisher_rast.ops import FisherScorer
            from models.SLAM.utils.recon_helpers import setup_camera
            W, H, sc, w2c = _family(case, oracle)
            K = intrinsics(W, H)
            cam = setup_camera(W, H, K, np.eye(4), device=gpu)
            ocam = oracle.setup_camera(W, H, K, np.eye(4))
            w2cs = _views(w2c, 3)
            args = (sc["means3D"], sc["colors"], sc["rotations"], sc["opacities"], sc["scales"])
            t = [torch.from_numpy(np.ascontiguousarray(a)).to(gpu) for a in args]
            cache[case] = dict(P=sc["means3D"].shape[0], w2cs=w2cs, cam=cam, t=t, scorers={}, ref={},
                               hess=lambda C, w: oracle.compute_hessian(ocam, w, *args, columns=C, arbiter=True))
        return cache[case]
    return get


def _scorer(f, C, **kw):
    from fisher_rast.ops import FisherScorer
    key = (C, tuple(sorted(kw.items())))
    if key not in f["scorers"]:
        f["scorers"][key] = FisherScorer(f["cam"], *f["t"], columns=C, **kw)
    return f["scorers"][key]


def _ref(f, C):
    """oracle / arbiter cur_H per view, H_inv = 1 / (H_train_o + 0.1) over views 1.., computed once per (family, columns)"""
    if C not in f["ref"]:
        cur = [f["hess"](C, w) for w in f["w2cs"]]
        cur_o = np.stack([h for h, _, _ in cur])
        cur_a = np.stack([h for _, h, _ in cur])
        vis_o = np.array([v for _, _, v in cur])
        H_train_o = cur_o[1:].sum(0, dtype=np.float32)
        H_inv_o = (np.float32(1.0) / (H_train_o + np.float32(0.1))).astype(np.float32)
        ent = [_entry_tolerance(cur_o[v], cur_a[v], C) for v in range(len(cur))]
        f["ref"][C] = dict(cur_o=cur_o, cur_a=cur_a, vis_o=vis_o, H_inv_o=H_inv_o, tol_entry=np.stack([e[0] for e in ent]),
                           r_G=np.stack([e[1] for e in ent]))
    return f["ref"][C]


def _want_tol(ref, weight):
    """want [V, P] and tol [V, P] for a weight [P, C] or [V, P, C] (the entry rule through the positive-weighted sum)"""
    w = weight.astype(np.float64)
    w = w[None] if w.ndim == 2 else w
    want = (ref["cur_o"].astype(np.float64) * w).sum(-1)
    tol = (ref["tol_entry"] * w).sum(-1) + 1e-7 * np.abs(want).max()
    return want, tol


def _k_needed(got, ref, weight, C):
    """the multiple of r_G the worst (view, Gaussian) pair needed beyond the flat part of the rule (reported)"""
    w = weight.astype(np.float64)
    w = w[None] if w.ndim == 2 else w
    o = np.abs(ref["cur_o"].astype(np.float64))
    want = (ref["cur_o"].astype(np.float64) * w).sum(-1)
    flat = (1e-4 * o * w).sum(-1) + (1e-7 * np.abs(ref["cur_o"].astype(np.float64)).max(axis=(1, 2), keepdims=True) * w).sum(-1) \
        + 1e-7 * np.abs(want).max()
    per_k = (ref["r_G"] * o * w).sum(-1)
    excess = np.abs(got - want) - flat
    return float(np.where((excess > 0) & (per_k > 0), excess / np.maximum(per_k, 1e-300), 0.0).max())


def _check(got, want, tol, what):
    bad = np.abs(got - want) > tol
    assert not bad.any(), (what, int(bad.sum()), float((np.abs(got - want) / np.maximum(tol, 1e-300)).max()))


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("case", FAMILIES)
def test_point_scores_against_the_oracle(family, gpu, case, columns):
    f = family(case)
    C, V, P = columns, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    want, tol = _want_tol(ref, ref["H_inv_o"])
    n_wide = int((ref["r_G"] > 2e-5).sum())
    assert n_wide <= 0.02 * V * P, (case, n_wide)
    sc = _scorer(f, C)
    r = sc.point_scores(torch.from_numpy(f["w2cs"]).to(gpu), torch.from_numpy(ref["H_inv_o"]).to(gpu))
    got = r["point_scores"].cpu().numpy().astype(np.float64)
    print(f"[{case}-{C}] K needed {_k_needed(got, ref, ref['H_inv_o'], C):.2f} of K_DEV {K_DEV[C]} (cap {WIDEN_CAP}), widened pairs {n_wide} of {V * P}, "
          f"worst |err| / tol {float((np.abs(got - want) / tol).max()):.3f}")
    assert np.array_equal(r["vis_count"].cpu().numpy(), ref["vis_o"])
    _check(got, want, tol, (case, C))
    s = r["scores"].cpu().numpy().astype(np.float64)
    print(f"[{case}-{C}] scores rel err {rel_err(s, want.sum(1)):.2e}")
    assert rel_err(s, want.sum(1)) < 1e-4, (case, s, want.sum(1))
    assert np.array_equal(r["point_max"].cpu().numpy(), r["point_scores"].cpu().numpy().max(0))


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("case", ["general", "crowded_tile"])
def test_packed_key_lists_give_the_same_scores(family, gpu, case, columns):
    """tile_capacity = 0: packed lists and the 96-byte records (the other form of the front end and of the tile kernel)"""
    f = family(case)
    ref = _ref(f, columns)
    want, tol = _want_tol(ref, ref["H_inv_o"])
    sc = _scorer(f, columns, tile_capacity=0)
    r = sc.point_scores(torch.from_numpy(f["w2cs"]).to(gpu), torch.from_numpy(ref["H_inv_o"]).to(gpu))
    assert np.array_equal(r["vis_count"].cpu().numpy(), ref["vis_o"])
    _check(r["point_scores"].cpu().numpy().astype(np.float64), want, tol, (case, columns, "packed"))
    assert rel_err(r["scores"].cpu().numpy().astype(np.float64), want.sum(1)) < 1e-4


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("case", ["general", "border", "ragged"])
def test_point_scores_against_the_out_h_route(family, gpu, case, columns):
    """the library's own other route: (cur * H_inv).sum(-1) of a per-view out_H launch.  Each is within `tol` of the oracle."""
    f = family(case)
    C, V, P = columns, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    _, tol = _want_tol(ref, ref["H_inv_o"])
    sc = _scorer(f, C)
    w2c = torch.from_numpy(f["w2cs"]).to(gpu)
    H_inv = torch.from_numpy(ref["H_inv_o"]).to(gpu)
    cur = torch.zeros((V, P, C), device=gpu)
    sc.run(w2c, out_H=cur, out_H_per_view=True)
    other = (cur.double() * H_inv.double()[None]).sum(-1).cpu().numpy()
    got = sc.point_scores(w2c, H_inv)["point_scores"].cpu().numpy().astype(np.float64)
    _check(got, other, 2.0 * tol, (case, C))


def test_identities_are_exact(family, gpu):
    f = family("general")
    C, V, P = 4, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    sc = _scorer(f, C)
    w2c = torch.from_numpy(f["w2cs"]).to(gpu)
    H_inv = torch.from_numpy(ref["H_inv_o"]).to(gpu)
    never = ~(np.stack([np.abs(ref["cur_o"][v]).sum(1) > 0 for v in range(V)]).any(0))
    g = torch.Generator().manual_seed(3)
    base = None
    for init in (torch.zeros((P,)), torch.rand((P,), generator=g) * 2e-3):
        pm = init.clone().to(gpu)
        out = torch.full((V, P), float("nan"), device=gpu)
        r = sc.point_launch(w2c, H_inv, out=out, point_max=pm)
        assert int(r["status"].cpu()[1]) == 0
        assert r["point_max"] is pm and r["point_scores"].data_ptr() == out.data_ptr()
        o = out.cpu()
        assert not torch.isnan(o).any() and (o >= 0).all()
        want = torch.maximum(init, o.max(0).values)
        assert torch.equal(pm.cpu().view(torch.int32), want.view(torch.int32))
        base = r["scores"].cpu() if base is None else base
        assert torch.equal(r["scores"].cpu().view(torch.int32), base.view(torch.int32))       # two calls: the same bits
    # Gaussians that no view sees (radius 0 everywhere: no entry of cur_H) keep their init; only the maximum asked for
    vis_any = np.zeros(P, bool)
    for v in range(V):
        one = sc.point_launch(w2c[v:v + 1], H_inv)
        assert torch.equal(one["scores"].cpu().view(torch.int32), base[v:v + 1].view(torch.int32))   # alone == inside the batch
        vis_any |= (one["point_scores"][0] > 0).cpu().numpy()
    assert never.sum() > 0 and not (vis_any & never).any()
    init = torch.rand((P,), generator=g) * 2e-3
    pm = init.clone().to(gpu)
    r = sc.point_launch(w2c, H_inv, per_view=False, point_max=pm)
    assert r["point_scores"] is None
    assert torch.equal(pm.cpu()[torch.from_numpy(never)], init[torch.from_numpy(never)])


def test_chunks_of_views_compose(family, gpu):
    f = family("crowded_tile")
    C, V, P = 11, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    want, tol = _want_tol(ref, ref["H_inv_o"])
    sc = _scorer(f, C)
    w2c = torch.from_numpy(f["w2cs"]).to(gpu)
    H_inv = torch.from_numpy(ref["H_inv_o"]).to(gpu)
    whole = sc.point_scores(w2c, H_inv, per_view=False)["point_max"].cpu().numpy().astype(np.float64)
    pm = torch.zeros((P,), device=gpu)
    for v in range(V):
        sc.point_scores(w2c[v:v + 1], H_inv, per_view=False, point_max=pm)
    parts = pm.cpu().numpy().astype(np.float64)
    # each side is within the rounding of its float atomics of the same sums: the rule of the oracle test bounds the difference
    tol_max = tol.max(0)
    assert (np.abs(whole - parts) <= tol_max).all()
    assert (np.abs(whole - want.max(0)) <= tol_max).all()
    # ... and chunking inside point_scores (one view per launch) is the same composition
    small = _scorer(f, C, tile_capacity=0)
    budget, small.WORKSPACE_BUDGET = small.WORKSPACE_BUDGET, 1
    try:
        assert small.max_views_per_launch() == 1
        r = small.point_scores(w2c, H_inv)
    finally:
        small.WORKSPACE_BUDGET = budget
    _check(r["point_scores"].cpu().numpy().astype(np.float64), want, tol, "chunked")
    assert np.array_equal(r["vis_count"].cpu().numpy(), ref["vis_o"]) and r["scores"].shape == (V,)


@pytest.mark.parametrize("columns", [4, 11])
@pytest.mark.parametrize("case", ["general", "border"])
def test_per_view_h_inv(family, gpu, case, columns):
    f = family(case)
    C, V, P = columns, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    g = torch.Generator().manual_seed(5)
    Hv = (torch.rand((V, P, C), generator=g) * 3.0 + 0.05)
    want, tol = _want_tol(ref, Hv.numpy())
    r = _scorer(f, C).point_scores(torch.from_numpy(f["w2cs"]).to(gpu), Hv.to(gpu), H_inv_per_view=True)
    _check(r["point_scores"].cpu().numpy().astype(np.float64), want, tol, (case, C, "per view"))
    assert rel_err(r["scores"].cpu().numpy().astype(np.float64), want.sum(1)) < 1e-4


def test_overflow_sets_status_and_writes_nothing(family, gpu):
    from fisher_rast.ops import FisherScorer
    f = family("general")
    C, V, P = 4, len(f["w2cs"]), f["P"]
    ref = _ref(f, C)
    want, tol = _want_tol(ref, ref["H_inv_o"])
    w2c = torch.from_numpy(f["w2cs"]).to(gpu)
    H_inv = torch.from_numpy(ref["H_inv_o"]).to(gpu)
    # a fixed key segment shorter than the longest tile list, and packed lists in a key buffer too small
    for kw in (dict(tile_capacity=16), dict(tile_capacity=0)):
        s = FisherScorer(f["cam"], *f["t"], columns=C, **kw)
        if kw["tile_capacity"] == 0:
            s.per_view_capacity = 16
        out = torch.full((V, P), 7.0, device=gpu)
        pm = torch.full((P,), 5.0, device=gpu)
        r = s.point_launch(w2c, H_inv, out=out, point_max=pm)
        st = r["status"].cpu().numpy()
        assert st[1] == 1 and (st[3] == 1) == (kw["tile_capacity"] > 0), (kw, st)
        assert (out.cpu().numpy() == 7.0).all() and (pm.cpu().numpy() == 5.0).all()
        # ... and point_scores grows the buffer and redoes the batch
        got = s.point_scores(w2c, H_inv)
        _check(got["point_scores"].cpu().numpy().astype(np.float64), want, tol, ("regrown", kw))
        assert np.array_equal(got["vis_count"].cpu().numpy(), ref["vis_o"])


def test_overflow_through_the_c_abi_leaves_every_output_byte(family, gpu):
    from fisher_rast import _lib
    from fisher_rast._lib import FisherCfg
    f = family("general")
    C, V, P = 4, len(f["w2cs"]), f["P"]
    sc = _scorer(f, C)
    lib = _lib.load()
    w2c = torch.from_numpy(f["w2cs"]).to(gpu).contiguous()
    H_inv = torch.from_numpy(_ref(f, C)["H_inv_o"]).to(gpu)
    R = 64                                                   # far fewer key slots than tile instances
    ws = torch.empty((int(lib.fr_fisher_point_workspace_bytes(P, sc.W, sc.H, V, R, C)),), dtype=torch.uint8, device=gpu)
    out = torch.full((V, P), 7.0, device=gpu)
    pm = torch.full((P,), 5.0, device=gpu)
    scores = torch.full((V,), 3.0, device=gpu)
    status = torch.zeros((4,), dtype=torch.int32, device=gpu)
    fc = FisherCfg()
    fc.n_views, fc.columns, fc.dL_dpix = V, C, 1e-3
    fc.w2c = ctypes.c_void_p(w2c.data_ptr())
    fc.H_inv = ctypes.c_void_p(H_inv.data_ptr())
    fc.out_scores = ctypes.c_void_p(scores.data_ptr())
    with torch.cuda.device(gpu):
        rc = lib.fr_fisher_point_views(ctypes.byref(sc.cfg), ctypes.byref(sc.g), ctypes.byref(fc), ctypes.c_void_p(out.data_ptr()),
                                       ctypes.c_void_p(pm.data_ptr()), ws.data_ptr(), ws.numel(), R, status.data_ptr(),
                                       ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0, lib.fr_last_error()
    st = status.cpu().numpy()
    assert st[1] == 1 and st[0] > R
    assert (out.cpu().numpy() == 7.0).all() and (pm.cpu().numpy() == 5.0).all() and (scores.cpu().numpy() == 3.0).all()


def test_empty_map_is_a_valid_call(gpu):
    """P = 0 through the C ABI (FisherScorer does not take an empty map): scores and counts are zeroed, status is clean"""
    from fisher_rast import _lib
    from fisher_rast._lib import FisherCfg, RasterCfg
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    from scenes import random_scene
    W, H, V = 80, 48, 2
    cam = setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)
    sc0 = random_scene(1, 3, scale=0.08)
    one = FisherScorer(cam, *[torch.from_numpy(np.ascontiguousarray(sc0[k])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")])
    lib = _lib.load()
    cfg = RasterCfg.from_buffer_copy(one.cfg)
    cfg.P = 0
    w2c = torch.from_numpy(_views(np.eye(4, dtype=np.float32), V)).to(gpu).contiguous()
    dummy = torch.full((4,), 9.0, device=gpu)
    scores = torch.full((V,), 3.0, device=gpu)
    vis = torch.full((V,), 7, dtype=torch.int32, device=gpu)
    status = torch.full((4,), 7, dtype=torch.int32, device=gpu)
    fc = FisherCfg()
    fc.n_views, fc.columns, fc.dL_dpix = V, 4, 1e-3
    fc.w2c = ctypes.c_void_p(w2c.data_ptr())
    fc.H_inv = ctypes.c_void_p(dummy.data_ptr())
    fc.out_scores = ctypes.c_void_p(scores.data_ptr())
    fc.out_vis_count = vis.data_ptr()
    with torch.cuda.device(gpu):
        rc = lib.fr_fisher_point_views(ctypes.byref(cfg), ctypes.byref(one.g), ctypes.byref(fc), None, ctypes.c_void_p(dummy.data_ptr()),
                                       None, 0, 0, status.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream))
    assert rc == 0, lib.fr_last_error()
    assert (scores.cpu().numpy() == 0).all() and (vis.cpu().numpy() == 0).all() and (status.cpu().numpy() == 0).all()
    assert (dummy.cpu().numpy() == 9.0).all()


@pytest.mark.parametrize("P", [1, 257, 1000])
def test_any_number_of_gaussians(gpu, oracle, P):
    """one Gaussian, P that is no multiple of 256: valid calls, the same numbers as the out_H route"""
    from fisher_rast.ops import FisherScorer
    from models.SLAM.utils.recon_helpers import setup_camera
    from scenes import random_scene
    W, H = 80, 48
    cam = setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)
    sc0 = random_scene(max(P, 1), 3, scale=0.08)
    t = [torch.from_numpy(np.ascontiguousarray(sc0[k][:P])).to(gpu) for k in ("means3D", "colors", "rotations", "opacities", "scales")]
    s = FisherScorer(cam, *t, columns=4)
    w2c = torch.from_numpy(_views(np.eye(4, dtype=np.float32), 2)).to(gpu)
    H_inv = torch.full((P, 4), 2.0, device=gpu)
    r = s.point_scores(w2c, H_inv)
    assert r["point_scores"].shape == (2, P) and r["point_max"].shape == (P,) and r["scores"].shape == (2,)
    cur = torch.zeros((2, P, 4), device=gpu)
    s.run(w2c, out_H=cur, out_H_per_view=True)
    other = (cur.double() * 2.0).sum(-1).cpu().numpy()
    got = r["point_scores"].cpu().numpy().astype(np.float64)
    # (a well-conditioned random scene: each route is within 1e-4 of the exact sums, relative to the largest)
    assert np.abs(got - other).max() <= 2e-4 * np.abs(other).max() + 1e-30
    assert np.array_equal(r["point_max"].cpu().numpy(), r["point_scores"].cpu().numpy().max(0))


from test_gpu_fisher_parity import config1  # noqa: E402,F401  (the fixture: BASELINE.json configs[0], 10k Gaussians, 8 views of 256 x 256)


@pytest.mark.parametrize("cls_name,columns", [("GaussianSLAM", 4), ("GaussianObjectSLAM", 11)])
def test_pose_eval_points_on_the_slam_surface(config1, gpu, cls_name, columns):  # noqa: F811
    import models.gaussian_slam as mgs
    from fisher_rast import distributed as D
    c = config1
    P, V = c["P"], c["V"]
    slam = getattr(mgs, cls_name)(params={k: v.clone() for k, v in c["params"].items()}, intrinsics=c["K"], width=c["W"], height=c["H"],
                                  device=gpu)
    for w in c["kf_w2c"]:
        slam.add_keyframe(w.to(gpu))
    poses = [p.to(gpu) for p in c["c2w"]]
    want_scores, want_c2w = slam.pose_eval(poses, random_gaussian_params=None)
    scores, c2ws, best, point = slam.pose_eval_points(poses, random_gaussian_params=None, per_view=True)
    assert scores.device.type == "cpu" and scores.dtype == torch.float32 and scores.shape == (V,)
    assert torch.equal(c2ws, want_c2w) and best.shape == (P,) and best.device == gpu and point.shape == (V, P)
    assert len(slam.pose_eval_points(poses)) == 3
    assert rel_err(scores.numpy(), want_scores.numpy()) < 1e-4
    assert torch.equal(best, point.max(0).values)
    # the per-view route on the same scorer and the same H_inv: every pair within twice the flat rule (a well-conditioned map: no
    # Gaussian's reference chain is widened here), relative to the entry sums the rule is stated on
    scorer = slam._scorer(None)
    H_inv = torch.reciprocal(slam.compute_H_train() + slam.H_TRAIN_REG)
    w2c = torch.linalg.inv(torch.stack(poses))
    cur = torch.zeros((V, P, columns), device=gpu)
    scorer.run(w2c, out_H=cur, out_H_per_view=True)
    other = (cur.double() * H_inv.double()[None]).sum(-1)
    tol2 = 2.0 * ((1e-4 * cur.double().abs() + 1e-7 * cur.double().abs().amax(dim=(1, 2), keepdim=True)) * H_inv.double()[None]).sum(-1) \
        + 2e-7 * other.abs().max()
    assert bool(((point.double() - other).abs() <= tol2).all()), float(((point.double() - other).abs() / tol2).max())
    # sharded_point_score_max at world size 1: the fused route against today's
    a = D.sharded_point_score_max(scorer, w2c, H_inv)
    b = D.sharded_point_score_max(scorer, w2c, H_inv, fused=True)
    assert bool(((a.double() - b.double()).abs() <= tol2.amax(0)).all())
    assert bool(((b.double() - other.amax(0)).abs() <= tol2.amax(0)).all())
