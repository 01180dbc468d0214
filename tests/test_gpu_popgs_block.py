"""-m gpu: the POp-GS block stage (fr_raster_cfg.ext of fr_fisher_views; csrc/fr_popgs_block.hip).

SCORE on the synthetic cases of tests/popgs_block_cases.py against the binary64 NumPy restatement within the derived bound (the CPU test
shows the g++ harness within it on the same cases); determinism; sentinels round every output and an exactly-sized workspace; stream
order; VISIBLE against `radii > 0` of the single-view rasteriser; PRIOR against compute_H_train_blocks(fused=False); the fused
pose_eval_popgs_blocks end to end against the restatement on the rows and the prior it used.

Measured on MI355X (largest |error| / bound over the poses of a case): written by the tests to stdout (-s)."""
import ctypes

import numpy as np
import pytest
import torch

import popgs_block_cases as pc


def go_visible_masks(slam, w2cs):
    import models.SLAM.gaussian_object as go
    return go.visible_masks(slam, w2cs)

pytestmark = pytest.mark.gpu

GUARD = 64
FILL = 0xA5


@pytest.fixture(scope="module")
def lib(gpu):
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


class Guarded:
    """a device buffer of `nbytes` with GUARD bytes of sentinel on either side"""

    def __init__(self, nbytes, dev):
        self.buf = torch.full((nbytes + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.n = nbytes

    @property
    def ptr(self):
        return self.buf.data_ptr() + GUARD

    def view(self, dtype):
        return self.buf[GUARD:GUARD + self.n].view(dtype)

    def intact(self):
        return bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + self.n:] == FILL).all())


def score_call(lib, case, criterion, dev, poses=None):
    """one SCORE call with vis_in on the current stream, every buffer guarded and the workspace exactly sized.
    poses: a slice of the case's poses (default all).  Returns dict(scores f64, matched i32, status i32 [4], guards)."""
    from fisher_rast import _lib
    K, P, n, d = case["K"], case["P"], case["n"], case["d"]
    sl = slice(0, case["poses"]) if poses is None else poses
    rows = torch.from_numpy(case["rows"].reshape(case["poses"], K, P, 11)[sl]).to(dev).contiguous()
    vis = torch.from_numpy(case["vis"][sl]).to(dev).contiguous()
    V = int(rows.shape[0])
    prior, idx = torch.from_numpy(case["prior"]).to(dev), torch.from_numpy(case["idx"]).to(dev)
    scores, matched, status = Guarded(8 * V, dev), Guarded(4 * V, dev), Guarded(16, dev)
    ws = Guarded(_lib.popgs_block_workspace_bytes(P, V), dev)
    cfg, fc, ext = _lib.RasterCfg(), _lib.FisherCfg(), _lib.RasterExt()
    cfg.P = P
    fc.n_views, fc.columns, fc.out_H, fc.out_H_view_stride = V * K, 11, rows.data_ptr(), 11 * P
    ext.kind, ext.mode, ext.K, ext.n, ext.lam, ext.criterion = _lib.FR_EXT_POPGS_BLOCK, _lib.FR_POPGS_BLOCK_SCORE, K, n, case["lam"], criterion
    ext.use_opacity, ext.use_rot, ext.use_scale = (int(case["flags"][k]) for k in ("use_opacity", "use_rot", "use_scale"))
    ext.vis_in, ext.prior_blocks, ext.prior_idx = vis.data_ptr(), prior.data_ptr(), idx.data_ptr()
    ext.out_scores, ext.out_matched = scores.ptr, matched.ptr
    cfg.ext = ctypes.pointer(ext)
    with torch.cuda.device(dev):
        rc = lib.fr_fisher_views(ctypes.byref(cfg), None, ctypes.byref(fc), ws.ptr, ws.n, 0, status.ptr,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.fr_last_error()
    guards = (scores, matched, status, ws)
    return dict(scores=scores.view(torch.float64), matched=matched.view(torch.int32), status=status.view(torch.int32), guards=guards,
                keep=(rows, vis, prior, idx))


_restated = {}


def restated(name, kw, criterion):
    """the restatement of a case, computed once and shared"""
    key = (name, criterion)
    if key not in _restated:
        case = pc.make_case(**kw)
        _restated[key] = (case, pc.restate(case, criterion))
    return _restated[key]


# ---- SCORE on synthetic rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,kw", pc.SCORE_CASES, ids=[c[0] for c in pc.SCORE_CASES])
@pytest.mark.parametrize("criterion", [pc.TOPT, pc.DOPT], ids=["topt", "dopt"])
def test_score_within_the_bound(lib, gpu, name, kw, criterion):
    case, want = restated(name, kw, criterion)
    r = score_call(lib, case, criterion, gpu)
    torch.cuda.synchronize()
    assert np.array_equal(r["matched"].cpu().numpy(), want["matched"])
    assert r["status"].cpu().tolist() == [int(want["matched"].sum()), 0, 0, 0]
    ratio = pc.check_scores(r["scores"].cpu().numpy(), want, f"{name}/{'dt'[criterion == pc.TOPT]}opt")
    print(f"RATIO {name} criterion {criterion}: {ratio:.4f} of the bound (largest kappa {want['kappa']:.3g})")
    assert all(g.intact() for g in r["guards"])


def test_unsorted_out_of_range_no_match_indefinite(lib, gpu):
    case = pc.make_case(11, 1100, 3, 2, 300, pc.FULL, unsorted=True)
    assert (np.diff(case["idx"]) < 0).any()
    case["idx"][7], case["idx"][190] = 1100, -1
    case["vis"][2, :] = 0
    rng = np.random.default_rng(3)
    case["prior"][4] = pc.indefinite_block(rng, 11)
    case["rows"][:, case["idx"][4], :] *= 1e-3
    case["vis"][:2, case["idx"][4]] = 1
    for criterion in (pc.TOPT, pc.DOPT):
        want = pc.restate(case, criterion)
        r = score_call(lib, case, criterion, gpu)
        torch.cuda.synchronize()
        st = r["status"].cpu().tolist()
        assert st == [int(want["matched"].sum()), 0, 2 if criterion == pc.TOPT else 4, 2]
        assert np.array_equal(r["matched"].cpu().numpy(), want["matched"]) and want["matched"][2] == 0
        got = r["scores"].cpu().numpy()
        assert got[2] == -np.inf
        pc.check_scores(got, want, "special")
        assert all(g.intact() for g in r["guards"])


def test_zero_rows_score_exactly_zero_under_dopt(lib, gpu):
    case = pc.make_case(5, 1100, 3, 3, 500, pc.FULL)
    case["rows"][:] = 0.0
    r = score_call(lib, case, pc.DOPT, gpu)
    torch.cuda.synchronize()
    assert int(r["matched"].sum()) > 0
    assert r["scores"].cpu().tolist() == [0.0, 0.0, 0.0]


def test_same_bits_twice_and_alone_as_in_the_batch(lib, gpu):
    for criterion in (pc.TOPT, pc.DOPT):
        case, _ = restated("n1000", dict(pc.SCORE_CASES)["n1000"], criterion)
        a = score_call(lib, case, criterion, gpu)
        b = score_call(lib, case, criterion, gpu)
        one = score_call(lib, case, criterion, gpu, poses=slice(1, 2))
        torch.cuda.synchronize()
        assert torch.equal(a["scores"].view(torch.int64), b["scores"].view(torch.int64)) and torch.equal(a["matched"], b["matched"])
        assert torch.equal(one["scores"].view(torch.int64), a["scores"][1:2].view(torch.int64)) and int(one["matched"][0]) == int(a["matched"][1])


def test_stream_order(lib, gpu):
    """one call on a non-default stream behind torch work that produces its inputs: the default stream's bits"""
    case, _ = restated("n257", dict(pc.SCORE_CASES)["n257"], pc.DOPT)
    ref = score_call(lib, case, pc.DOPT, gpu)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(side):
        big = torch.randn((2048, 2048), device=gpu)
        for _ in range(8):
            big = big @ big * 1e-3                                        # work the call has to wait behind
        r = score_call(lib, case, pc.DOPT, gpu)
    side.synchronize()
    assert torch.equal(r["scores"].view(torch.int64), ref["scores"].view(torch.int64)) and torch.equal(r["matched"], ref["matched"])


# ---- the scene of the parity tests (BASELINE configs[0]) -------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scene(gpu):
    from fisher_rast import synthetic
    import models.gaussian_slam as mgs
    P, W, H = 10000, 256, 256
    params = synthetic.room_shell(P, seed=1)
    K = synthetic.intrinsics(W, H)
    c2w = synthetic.candidate_poses(8, seed=1)
    kf_w2c = synthetic.invert_rigid(synthetic.candidate_poses(4, seed=101))
    slam = mgs.GaussianObjectSLAM(params=params, intrinsics=K, width=W, height=H, device=gpu)
    for kf in kf_w2c[:3]:
        slam.add_keyframe(kf)
    return dict(P=P, W=W, H=H, slam=slam, c2w=c2w, w2c=synthetic.invert_rigid(c2w), kf_w2c=kf_w2c[:3])


def _draws(n, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, 3, H, W), generator=g)


def test_visible_equals_the_rasterisers_radii(scene, gpu):
    slam = scene["slam"]
    w2cs = torch.cat([scene["w2c"], scene["kf_w2c"]]).to(gpu)
    mask, counts = go_visible_masks(slam, w2cs)
    assert mask.dtype == torch.bool and tuple(mask.shape) == (11, scene["P"]) and counts.dtype == torch.int32
    rows = torch.zeros((11, scene["P"], 11), device=gpu)
    res = slam._scorer().run(w2cs, out_H=rows, out_H_per_view=True)
    assert torch.equal(counts, res["vis_count"]) and torch.equal(mask.sum(dim=1).int(), counts)
    for v in range(11):
        idx = slam._visible_indices(w2cs[v])
        assert torch.equal(torch.nonzero(mask[v]).reshape(-1), idx), v
    assert len(set(counts.tolist())) > 1 and 0 < int(counts.min()) and int(counts.max()) < scene["P"]


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("flags", [pc.FLAG_SETS[-1], pc.FLAG_SETS[2]], ids=pc.flag_id)
def test_prior_against_the_unfused_route(scene, gpu, K, flags, monkeypatch):
    """Both routes are given the rows of ONE probe launch: fr_fisher_views accumulates a row with floating-point atomics, so two
    launches of the same probes differ in the last bit of some entries (measured: ~1e3 of 1.1e5 entries per keyframe, 3e-7 relative)
    and no comparison of two launches can be exact.  On the same rows the stage is the torch chain bit for bit at K = 1.

    K = 2: the tolerance the issue sets, 2 * 2^-24 * sum_k |g_a g_b| / K per keyframe.  torch's einsum runs, per keyframe, the chain
    b = fma(g_a, g_b, b) from 0 with k ascending (measured on MI355X: bit-equal), and so does the stage: the difference is 0."""
    slam = scene["slam"]
    kf = scene["kf_w2c"].to(gpu)
    zs = list(_draws(K, scene["H"], scene["W"], 40 + K))
    rows, vis = slam._pose_probe_rows(kf, K, zs * 3)

    def pinned(w2cs, K_, zs_=None):
        w2cs = w2cs.reshape(-1, 4, 4)
        sel = [next(f for f in range(3) if torch.equal(w2cs[v], kf[f])) for v in range(int(w2cs.shape[0]))]
        assert K_ == K
        return rows[sel], vis[sel]
    monkeypatch.setattr(slam, "_pose_probe_rows", pinned, raising=False)
    Hm, idx = slam.compute_H_train_blocks(K=K, zs=zs, **flags)
    Hf, idf = slam.compute_H_train_blocks(K=K, fused=True, zs=zs, **flags)
    monkeypatch.undo()
    mask, counts = go_visible_masks(slam, kf)
    assert len(set(counts.tolist())) == 3, "the keyframes' visible counts must differ: the truncation is what is tested"
    n = int(counts.min())
    assert Hf.shape == Hm.shape == (n, pc_d(flags), pc_d(flags)) and idf.dtype == idx.dtype
    assert torch.equal(idf, idx)
    if K == 1:
        assert torch.equal(Hf, Hm)
        return
    # |difference| <= 2 * 2^-24 * sum_k |g_a g_b| / K per keyframe, at that keyframe's r-th visible Gaussian
    cols = pc.columns(**flags)
    tol = torch.zeros_like(Hm, dtype=torch.float64)
    for f in range(3):
        G = rows[f][:, torch.nonzero(mask[f]).reshape(-1)[:n]][:, :, cols].double().abs()
        tol += 2 * 2.0 ** -24 * torch.einsum("kvi,kvj->vij", G, G) / K
    err = (Hf.double() - Hm.double()).abs()
    print(f"PRIOR K={K}: largest |difference| / tolerance {float((err / tol.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= tol).all())


def geometry_call(lib, sc, mode, w2cs, K, rows, capacity, flags, dev):
    """one raw VISIBLE or PRIOR call on the scorer's camera and map: prior_blocks [capacity,d,d], prior_idx [capacity], out_vis,
    out_vis_count and status guarded, the workspace exactly sized"""
    from fisher_rast import _lib
    V, P, d = int(w2cs.shape[0]), sc.P, len(pc.columns(**flags))
    views = w2cs.repeat_interleave(K, dim=0).contiguous()
    blocks, idx = Guarded(4 * capacity * d * d, dev), Guarded(4 * capacity, dev)
    vis, counts, status = Guarded(V * P, dev), Guarded(4 * V, dev), Guarded(16, dev)
    ws = Guarded(_lib.popgs_block_workspace_bytes(P, V), dev)
    cfg, fc, ext = _lib.RasterCfg.from_buffer_copy(sc.cfg), _lib.FisherCfg(), _lib.RasterExt()
    fc.n_views, fc.columns, fc.w2c, fc.out_H_view_stride = V * K, 11, views.data_ptr(), 11 * P
    fc.out_H = None if rows is None else rows.data_ptr()
    ext.kind, ext.mode, ext.K, ext.n = _lib.FR_EXT_POPGS_BLOCK, mode, K, capacity
    ext.use_opacity, ext.use_rot, ext.use_scale = (int(flags[k]) for k in ("use_opacity", "use_rot", "use_scale"))
    ext.out_vis, ext.out_vis_count = vis.ptr, counts.ptr
    if mode == _lib.FR_POPGS_BLOCK_PRIOR:
        ext.prior_blocks, ext.prior_idx = blocks.ptr, idx.ptr
    cfg.ext = ctypes.pointer(ext)
    with torch.cuda.device(dev):
        rc = lib.fr_fisher_views(ctypes.byref(cfg), ctypes.byref(sc.g), ctypes.byref(fc), ws.ptr, ws.n, 0, status.ptr,
                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, lib.fr_last_error()
    torch.cuda.synchronize()
    return dict(blocks=blocks.view(torch.float32).reshape(capacity, d, d), idx=idx.view(torch.int32), vis=vis.view(torch.uint8).reshape(V, P),
                counts=counts.view(torch.int32), status=status.view(torch.int32), guards=(blocks, idx, vis, counts, status, ws), keep=views)


@pytest.mark.parametrize("flags", [pc.FLAG_SETS[-1], pc.FLAG_SETS[0]], ids=pc.flag_id)
def test_prior_and_visible_stay_inside_their_buffers(lib, scene, gpu, flags):
    """raw calls: sentinels round the prior outputs, the masks, the counts and the status word, and a workspace of exactly
    FR_POPGS_BLOCK_WS_BYTES.  A capacity (ext.n) below the smallest visible count writes the first ext.n rows alone and still reports
    the full n."""
    from fisher_rast import _lib
    slam, K = scene["slam"], 2
    sc = slam._scorer()
    kf = scene["kf_w2c"].to(gpu)
    rows, _ = slam._pose_probe_rows(kf, K, list(_draws(3 * K, scene["H"], scene["W"], 9)))
    Hm, idx = sc.popgs_block_prior(rows, kf, K, **flags)
    mask, counts = sc.visible(kf)
    n = int(counts.min())
    assert Hm.shape[0] == n > 7
    for capacity in (n, n - 7, 1):
        r = geometry_call(lib, sc, _lib.FR_POPGS_BLOCK_PRIOR, kf, K, rows, capacity, flags, gpu)
        assert r["status"].tolist() == [n, 0, 0, 0], capacity                       # the full n, whatever the capacity
        assert torch.equal(r["blocks"], Hm[:capacity]) and torch.equal(r["idx"], idx[:capacity])
        assert torch.equal(r["vis"].bool(), mask) and torch.equal(r["counts"], counts)
        assert all(g.intact() for g in r["guards"]), capacity
    # a capacity beyond n: the rows from n on keep the caller's bytes
    r = geometry_call(lib, sc, _lib.FR_POPGS_BLOCK_PRIOR, kf, K, rows, n + 5, flags, gpu)
    assert r["status"].tolist() == [n, 0, 0, 0] and torch.equal(r["blocks"][:n], Hm) and torch.equal(r["idx"][:n], idx)
    assert bool((r["blocks"][n:].contiguous().view(torch.uint8) == FILL).all()) and bool((r["idx"][n:].contiguous().view(torch.uint8) == FILL).all())
    assert all(g.intact() for g in r["guards"])
    # VISIBLE alone, rows null: a pose more than PRIOR had, so another workspace size
    w2cs = torch.cat([kf, scene["w2c"][:2].to(gpu)])
    m5, c5 = sc.visible(w2cs)
    r = geometry_call(lib, sc, _lib.FR_POPGS_BLOCK_VISIBLE, w2cs, 1, None, 1, flags, gpu)
    assert r["status"].tolist() == [0, 0, 0, 0] and torch.equal(r["vis"].bool(), m5) and torch.equal(r["counts"], c5)
    assert bool((r["vis"] <= 1).all()) and all(g.intact() for g in r["guards"])


def pc_d(flags):
    return len(pc.columns(**flags))


@pytest.mark.parametrize("conditioned", [False, True], ids=["lam1e-3", "lam-conditioned"])
@pytest.mark.parametrize("criterion", ["topt", "dopt"])
def test_fused_pose_eval_end_to_end(scene, gpu, criterion, conditioned, monkeypatch):
    """lam = 1e-3: the blocks' condition reaches 3e15 and the derived bound is wider than the terms, so that case checks the plumbing
    (the rows, prior and visibility the call used, the pairs per pose, -inf, shapes and types), not the values.  The conditioned case
    takes lam = 1e-6 of the largest absolute row sum of a prior from the same keyframes, which keeps kappa below 1e9 (asserted by the
    restatement): there the bound binds."""
    import models.SLAM.gaussian_object as go
    slam, K, V = scene["slam"], 2, 8
    lam, kappa_max = 1e-3, np.inf
    if conditioned:
        scale, _ = slam.compute_H_train_blocks(K=K, fused=True)
        lam, kappa_max = float(scale.abs().sum(dim=2).max()) * 1e-6, pc.KAPPA_MAX
    zs = _draws(V * K, scene["H"], scene["W"], 77).reshape(V, K, 3, scene["H"], scene["W"])
    seen = {}
    prior_fn, scores_fn, rows_fn = go._fused_block_prior, go._fused_block_scores, slam._pose_probe_rows

    def keep_prior(*a, **k):
        seen["prior"] = prior_fn(*a, **k)
        return seen["prior"]

    def keep_scores(*a, **k):
        seen["scores"] = scores_fn(*a, **k)
        return seen["scores"]

    def keep_rows(w2cs, K_, zs_=None):
        seen["rows"] = rows_fn(w2cs, K_, zs_)
        seen["w2cs"] = w2cs
        return seen["rows"]
    monkeypatch.setattr(go, "_fused_block_prior", keep_prior)
    monkeypatch.setattr(go, "_fused_block_scores", keep_scores)
    monkeypatch.setattr(slam, "_pose_probe_rows", keep_rows, raising=False)
    poses = [p.to(gpu) for p in scene["c2w"]]
    scores, c2ws = slam.pose_eval_popgs_blocks(poses, criterion=criterion, K=K, lam=lam, fused=True, zs=zs)
    monkeypatch.undo()
    assert scores.dtype == torch.float32 and scores.device.type == "cpu" and tuple(scores.shape) == (V,)
    assert tuple(c2ws.shape) == (V, 4, 4) and c2ws.dtype == torch.float32 and torch.equal(c2ws.cpu(), torch.stack(list(scene["c2w"])).float())
    assert torch.equal(scores, seen["scores"].float().cpu())
    Hm, idx = seen["prior"]
    rows = seen["rows"][0]                                                           # [V, K, P, 11]: one chunk at this size
    assert tuple(rows.shape) == (V, K, scene["P"], 11)
    mask, _ = go_visible_masks(slam, seen["w2cs"])
    case = dict(rows=rows.reshape(V * K, scene["P"], 11).cpu().numpy(), prior=Hm.cpu().numpy(), idx=idx.cpu().numpy().astype(np.int32),
                vis=mask.cpu().numpy().astype(np.uint8), lam=lam, K=K, P=scene["P"], flags=pc.FULL)
    crit = pc.TOPT if criterion == "topt" else pc.DOPT
    want = pc.restate(case, crit, kappa_max=kappa_max)
    ratio = pc.check_scores(seen["scores"].cpu().numpy(), want, f"end to end {criterion}")
    # the pairs per pose: the stage again on the rows, prior and poses the call used (the same bits, and its counts)
    again, pairs = slam._scorer().popgs_block_scores(rows, seen["w2cs"], K, Hm, idx, lam=lam, criterion=criterion)
    assert torch.equal(again.view(torch.int64), seen["scores"].view(torch.int64))
    assert np.array_equal(pairs.cpu().numpy(), want["matched"]) and (want["matched"] == 0).any() and (want["matched"] > 0).sum() >= 4
    assert np.array_equal(np.isinf(scores.numpy()), want["matched"] == 0)
    print(f"RATIO end to end {criterion} lam {lam:.3g}: {ratio:.4f} of the bound (largest kappa {want['kappa']:.3g}, pairs {want['matched'].tolist()})")
    # the binary32 LAPACK route on the same rows and prior: reported, not asserted
    old = []
    cols = pc.columns()
    for v in range(V):
        cur = torch.nonzero(mask[v]).reshape(-1)
        G = rows[v][:, cur][:, :, cols]
        Jb = torch.einsum("kvi,kvj->vij", G, G) / float(K)
        in_train, in_cur = torch.isin(idx, cur), torch.isin(cur, idx)
        old.append(float(slam._block_scores(Hm[in_train], Jb[in_cur], lam, criterion)))
    fin = np.isfinite(want["scores"])
    dev_old = np.abs(np.array(old)[fin] - want["scores"][fin]) / np.abs(want["scores"][fin])
    dev_new = np.abs(seen["scores"].cpu().numpy()[fin] - want["scores"][fin]) / np.abs(want["scores"][fin])
    print(f"OLD ROUTE {criterion} lam {lam:.3g}: relative deviation from binary64 NumPy, fused=False arithmetic {dev_old.max():.3e}, fused=True {dev_new.max():.3e}")


def test_scorer_api_computes_the_visibility_it_is_not_given(scene, gpu):
    slam = scene["slam"]
    sc = slam._scorer()
    w2cs = scene["w2c"][:3].to(gpu)
    K = 2
    rows, _ = slam._pose_probe_rows(w2cs, K, list(_draws(3 * K, scene["H"], scene["W"], 5)))
    kf_rows, _ = slam._pose_probe_rows(scene["kf_w2c"].to(gpu), K, list(_draws(3 * K, scene["H"], scene["W"], 6)))
    Hm, idx = sc.popgs_block_prior(kf_rows, scene["kf_w2c"].to(gpu), K)
    assert idx.dtype == torch.int32 and Hm.shape[0] == idx.shape[0] > 0
    mask, _ = sc.visible(w2cs)
    a, ma = sc.popgs_block_scores(rows, w2cs, K, Hm, idx, lam=1e-3, criterion="dopt")
    sta = sc.block_status.clone()
    b, mb = sc.popgs_block_scores(rows, w2cs, K, Hm, idx, lam=1e-3, criterion="dopt", vis=mask)
    assert a.dtype == torch.float64 and a.is_cuda and torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(ma, mb)
    assert torch.equal(sta, sc.block_status) and int(sta[0]) == int(ma.sum()) and int(sta[3]) == 0
    assert torch.equal(ma, (mask[:, idx.long()]).sum(dim=1).int())
    # a prior the poses do not see: -inf, nothing matched
    none = torch.zeros_like(mask)
    c, mc = sc.popgs_block_scores(rows, w2cs, K, Hm, idx, lam=1e-3, vis=none)
    assert bool(torch.isinf(c).all()) and bool((c < 0).all()) and int(mc.sum()) == 0
