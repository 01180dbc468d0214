"""-m gpu: the map edit (fr_map_edit_plan / fr_map_edit_apply / fr_map_edit_split_children, csrc/fr_mapedit.hip) and what is written
on it (remove_points / prune_gaussians / densify of models/SLAM/utils/slam_external.py).

Through the C ABI on guarded buffers: the three index lists and the status against nonzero of the masks, for every P at a wave or
workgroup edge and every mask family; a table of 25 arrays in one launch against the torch x[mask] / cat / repeat chain, bit for bit,
NaN payloads and -0 included; the split children against the g++ harness over the same header.  Then the product functions with a
real Adam against what the reference gave (tests/golden/reference_map_edit.npz), and one mapping iteration through the drop-in
rasteriser."""
import ctypes

import numpy as np
import pytest
import torch

import map_edit_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 64                    # words behind every buffer
GUARD_BITS = 0x5A5A5A5A
SIZES = [0, 1, 63, 64, 65, 256, 257, 4097, 70001]      # wave and workgroup edges; 70001: more than 256 count workgroups (two scan rounds)
FAMILIES = ["none", "all", "alternating", "run-over-edge", "random-10", "random-50", "random-90", "keep-null", "no-clone-no-split"]


@pytest.fixture(scope="module")
def edit_harness():
    return mc.build_harness()


@pytest.fixture(scope="module")
def gold():
    return mc.load_golden()


class _Guarded:
    """a device buffer of n 32-bit words, filled with the guard pattern (or `init`), with GUARD more words behind it"""

    def __init__(self, n, dev, init=None):
        self.buf = torch.full((n + GUARD,), GUARD_BITS, dtype=torch.int32, device=dev)
        if init is not None:
            self.buf[:n] = torch.from_numpy(np.ascontiguousarray(init).reshape(-1).view(np.int32)).to(dev)
        self.n = n

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, dtype=np.uint32):
        return self.buf[:self.n].cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.buf[self.n:] == GUARD_BITS).all())


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _masks(P, family):
    """(keep, clone, split) bool arrays or None"""
    rng = np.random.default_rng([P, FAMILIES.index(family), 20250602])
    i = np.arange(P)
    if family == "none":
        m = [np.zeros(P, bool)] * 3
    elif family == "all":
        m = [np.ones(P, bool)] * 3
    elif family == "alternating":
        m = [i % 2 == 0, i % 2 == 1, i % 3 == 0]
    elif family == "run-over-edge":                       # one run across the first workgroup edge (or the middle of a smaller map)
        c = 256 if P > 270 else P // 2
        m = [(i >= c - 7) & (i < c + 9), (i >= c - 1) & (i < c + 1), (i >= c - 70) & (i < c + 70)]
    elif family.startswith("random"):
        p = int(family.split("-")[1]) / 100
        m = [rng.uniform(size=P) < p for _ in range(3)]
    elif family == "keep-null":
        m = [None, rng.uniform(size=P) < 0.3, rng.uniform(size=P) < 0.3]
    else:
        m = [rng.uniform(size=P) < 0.6, None, None]
    return m


def _plan(dev, P, masks, short=0):
    """fr_map_edit_plan on guarded status and workspace: (return code, status [4], the three lists, guards intact, workspace)"""
    from fisher_rast import _lib
    lib = _lib.load()
    nws = int(lib.fr_map_edit_workspace_bytes(P))
    assert nws % 4 == 0 and nws >= 3 * _lib.edit_ws_list_stride(P)
    status, ws = _Guarded(_lib.FR_EDIT_STATUS_WORDS, dev), _Guarded(nws // 4, dev)
    held = [None if m is None else torch.from_numpy(m.astype(np.uint8) * np.uint8(3)).to(dev) for m in masks]     # any non-zero byte selects
    rc = lib.fr_map_edit_plan(P, *(None if h is None else h.data_ptr() for h in held), status.ptr, ws.ptr, nws - short, _stream(dev))
    torch.cuda.synchronize()
    st = status.get(np.int32)
    words = ws.get(np.int32)
    stride = _lib.edit_ws_list_stride(P) // 4
    lists = [words[k * stride:k * stride + max(int(st[k]), 0)].copy() for k in range(3)] if rc == 0 else None
    return rc, st, lists, status.intact() and ws.intact(), ws


def _want_lists(P, masks):
    keep, clone, split = masks
    return [np.arange(P, dtype=np.int32) if keep is None else np.flatnonzero(keep).astype(np.int32),
            np.flatnonzero(clone).astype(np.int32) if clone is not None else np.zeros(0, np.int32),
            np.flatnonzero(split).astype(np.int32) if split is not None else np.zeros(0, np.int32)]


@pytest.mark.parametrize("P", SIZES)
def test_plan_equals_nonzero_of_the_masks(gpu, P):
    for family in FAMILIES:
        masks = _masks(P, family)
        rc, st, lists, intact, _ = _plan(gpu, P, masks)
        want = _want_lists(P, masks)
        assert rc == 0 and intact, (family, rc)
        assert st.tolist() == [len(want[0]), len(want[1]), len(want[2]), 0], (family, st)
        for k in range(3):
            assert np.array_equal(lists[k], want[k]), (family, k)


COLS = (1, 3, 4, 16, 7)        # 7: a width the kernel divides by at run time


def _table(P, seed):
    """25 arrays of distinct bit patterns: (uint32 [P, cols], appended mode); NaN payloads, -0 and infinities among them"""
    rng = np.random.default_rng([P, seed])
    out = []
    for a in range(25):
        cols = COLS[a % 5]
        x = rng.integers(0, 2 ** 32, (P, cols), dtype=np.uint64).astype(np.uint32)
        if P:
            x.reshape(-1)[::7] = np.array([0x7FC00001, 0xFFC12345, 0x80000000, 0x7F800000, 0x7F812345, 0x00000001, 0xFF800000], np.uint32)[
                np.arange(x.reshape(-1)[::7].size) % 7]
        out.append((x, (a // 5 + a) % 2))
    return out


def _apply(dev, P, lists, n_into, ws, table):
    from fisher_rast import _lib
    lib = _lib.load()
    nk, nc, ns = (len(l) for l in lists)
    rows = nk + nc + n_into * ns
    srcs = [torch.from_numpy(x.view(np.int32)).to(dev) for x, _ in table]
    dsts = [_Guarded(rows * x.shape[1], dev) for x, _ in table]
    arr = (_lib.MapEditArray * len(table))(*[_lib.MapEditArray(s.data_ptr(), d.ptr, x.shape[1], mode) for s, d, (x, mode) in zip(srcs, dsts, table)])
    rc = lib.fr_map_edit_apply(arr, len(table), P, nk, nc, ns, n_into, ws.ptr, _stream(dev))
    torch.cuda.synchronize()
    return rc, srcs, dsts, rows


@pytest.mark.parametrize("P", SIZES)
def test_apply_equals_the_torch_chain_bit_for_bit(gpu, P):
    table = _table(P, 3)
    for family, n_into in (("random-50", 2), ("keep-null", 3), ("no-clone-no-split", 2), ("run-over-edge", 3), ("none", 2), ("all", 3)):
        masks = _masks(P, family)
        rc, st, lists, intact, ws = _plan(gpu, P, masks)
        assert rc == 0 and intact
        rc, srcs, dsts, rows = _apply(gpu, P, lists, n_into, ws, table)
        assert rc == 0, (family, rc)
        t = lambda m, default: torch.full((P,), default, dtype=torch.bool, device=gpu) if m is None else torch.from_numpy(m).to(gpu)
        keep, clone, split = t(masks[0], True), t(masks[1], False), t(masks[2], False)
        for (x, mode), src, dst in zip(table, srcs, dsts):
            tail = torch.cat((src[clone], src[split].repeat(n_into, 1)), dim=0)                     # the reference's chain, on the words
            want = torch.cat((src[keep], torch.zeros_like(tail) if mode == 1 else tail), dim=0)
            assert want.shape[0] == rows
            got = dst.buf[:dst.n].reshape(rows, x.shape[1])
            assert torch.equal(got, want), (family, x.shape, mode)
            assert dst.intact(), (family, "words past the last row")
            assert torch.equal(src.cpu(), torch.from_numpy(x.view(np.int32))), "a source was written"


@pytest.mark.parametrize("cols,n_into", [(3, 2), (1, 3)])
def test_split_children_against_the_harness(gpu, edit_harness, cols, n_into):
    from fisher_rast import _lib
    z, means, rot, logs = mc.sweep()
    n = (z.shape[0] // n_into) * n_into
    z, means, rot, logs = z[:n], means[:n], rot[:n], np.ascontiguousarray(logs[:n, :cols])
    want_means, want_logs = means.copy(), logs.copy()
    mc.harness_split(edit_harness, n_into, z, want_means, rot, want_logs)
    d_means, d_logs = _Guarded(n * 3, gpu, means), _Guarded(n * cols, gpu, logs)
    d_z, d_rot = _Guarded(n * 3, gpu, z), _Guarded(n * 4, gpu, rot)
    _lib.check(_lib.load().fr_map_edit_split_children(n // n_into, n_into, cols, d_z.ptr, d_means.ptr, d_rot.ptr, d_logs.ptr, _stream(gpu)),
               "fr_map_edit_split_children")
    torch.cuda.synchronize()
    assert all(g.intact() for g in (d_means, d_logs, d_z, d_rot))
    assert np.array_equal(d_z.get(), mc.bits(z).reshape(-1)) and np.array_equal(d_rot.get(), mc.bits(rot).reshape(-1))
    assert np.array_equal(d_means.get().reshape(n, 3), mc.bits(want_means)), "child means differ from the g++ build of the header"
    got_logs = d_logs.get(np.float32).reshape(n, cols)
    want64 = np.log(np.exp(logs.astype(np.float64)) / np.float64(mc.F(0.8 * n_into)))
    assert mc.log_scale_ok(got_logs, want64) and mc.log_scale_ok(want_logs, want64)
    # no child: nothing is launched or written
    _lib.check(_lib.load().fr_map_edit_split_children(0, n_into, cols, None, None, None, None, _stream(gpu)), "fr_map_edit_split_children")


def _device_edit(st, gpu):
    """the product's MapEdit over its device backend, with the case's recorded normal samples and call counters"""
    from models.SLAM.utils import slam_external as se

    class Backend(se.HipMapEditBackend):
        plans = applies = 0

        def plan(self, *a, **k):
            self.plans += 1
            return super().plan(*a, **k)

        def apply(self, *a, **k):
            self.applies += 1
            return super().apply(*a, **k)

        def randn(self, rows, like, generator=None):
            return torch.from_numpy(np.ascontiguousarray(st["z"][:rows])).to(like.device)

    backend = Backend()
    return se.MapEdit(backend), backend


@pytest.mark.parametrize("case", list(mc.CASES))
def test_product_functions_against_the_reference_vectors(gpu, gold, case):
    st = mc.state_of(case, gold)
    edit, backend = _device_edit(st, gpu)
    snap, params, variables, opt, before = mc.run_case(case, edit, st, gpu)
    torch.cuda.synchronize()
    mc.check_bookkeeping(params, variables, opt, before)
    assert all(params[k].is_cuda for k in mc.MAP_KEYS) and variables["denom"].is_cuda
    mc.compare_with_golden(case, st, snap, mc.golden_of(gold, case))
    fn = mc.CASES[case]["fn"]
    expect = {"remove_points": 1, "cat": 0, "densify": 2, "prune": 0 if case == "prune/off-beat-reset" else 1}[fn]
    assert backend.plans == expect == backend.applies


def test_module_level_functions_and_the_generator(gpu, gold):
    """the functions the module exports run on the device backend; densify draws its samples from the generator it is handed"""
    from models.SLAM.utils import slam_external as se
    st = mc.state_of("densify/n2", gold)
    outs = []
    for seed in (5, 5, 6):
        params, variables, opt = mc.build_inputs(st, gpu)
        g = torch.Generator(device=gpu).manual_seed(seed)
        params, variables = se.densify(params, variables, opt, 20, dict(mc.DENSIFY), generator=g)
        outs.append(params["means3D"].detach().cpu().numpy())
    want = mc.golden_of(gold, "densify/n2")
    child = want["child_index"] >= 0
    assert outs[0].shape == outs[2].shape == want["p/means3D"].shape
    assert np.array_equal(mc.bits(outs[0]), mc.bits(outs[1])) and not np.array_equal(mc.bits(outs[0])[child], mc.bits(outs[2])[child])
    assert np.array_equal(mc.bits(outs[0])[~child], mc.bits(want["p/means3D"])[~child])
    params, variables, opt = mc.build_inputs(st, gpu)
    m = torch.from_numpy(mc.removal_mask(mc.P_GOLDEN)).to(gpu)
    params, variables = se.remove_points(m, params, variables, opt)
    assert np.array_equal(mc.bits(params["means3D"].detach().cpu().numpy()), mc.bits(gold["remove/optimizer/p/means3D"]))


def _host_syncs(step):
    """synchronisations torch's sync debug mode reports during one call"""
    import warnings
    torch.cuda.synchronize()
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            step()
        finally:
            torch.cuda.set_sync_debug_mode("default")
    return sum("synchroniz" in str(w.message).lower() and "prototype" not in str(w.message).lower() for w in seen)


def test_one_host_read_per_stage(gpu, gold):
    """prune_gaussians reads the host once, densify twice (scene_radius, a float32 scalar on the device, rides with the counts)"""
    from models.SLAM.utils import slam_external as se
    st = mc.state_of("densify/n3-big", gold)
    cfg = mc.CASES["densify/n3-big"]["cfg"]
    params, variables, opt = mc.build_inputs(st, gpu)
    assert variables["scene_radius"].is_cuda
    g = torch.Generator(device=gpu).manual_seed(1)
    assert _host_syncs(lambda: se.densify(params, variables, opt, 20, dict(cfg), generator=g)) == 2
    params, variables, opt = mc.build_inputs(st, gpu)
    assert _host_syncs(lambda: se.prune_gaussians(params, variables, opt, 20, dict(mc.PRUNE, remove_big_after=0))) == 1
    assert params["means3D"].shape[0] == gold["prune/big/p/means3D"].shape[0] < mc.P_GOLDEN      # the caller's dict holds the edited map
    torch.cuda.synchronize()


def test_mapping_iteration_with_the_drop_in_rasteriser(gpu):
    """render -> loss -> backward -> prune_gaussians -> densify -> optimizer.step(), twice: the row counts the masks predict, the
    Adam state following the map, finite parameters"""
    from fisher_rast import synthetic
    from models.SLAM.utils import slam_external as se
    from models.SLAM.utils.recon_helpers import setup_camera
    from models.SLAM.utils.slam_helpers import render_rgb_depth_sil
    P, W, H = 5000, 64, 64
    params = {k: torch.nn.Parameter(v.to(gpu).contiguous().requires_grad_(True)) for k, v in synthetic.room_shell(P, seed=9).items()}
    opt = torch.optim.Adam([dict(params=[v], name=k, lr=1e-3) for k, v in params.items()])
    cam = setup_camera(W, H, synthetic.intrinsics(W, H), np.eye(4), device=gpu)
    w2c = synthetic.invert_rigid(synthetic.candidate_poses(1, seed=10))[0].to(gpu)
    variables = dict(max_2D_radius=torch.zeros(P, device=gpu), means2D_gradient_accum=torch.zeros(P, device=gpu), denom=torch.zeros(P, device=gpu),
                     timestep=torch.zeros(P, device=gpu), scene_radius=torch.tensor(3.0, device=gpu))
    prune_cfg = dict(mc.PRUNE, removal_opacity_threshold=0.3, remove_big_after=0)
    dens_cfg = dict(mc.DENSIFY, grad_thresh=0.0, removal_opacity_threshold=0.3, remove_big_after=0)
    plans = []

    class Backend(se.HipMapEditBackend):
        def plan(self, *a, **k):
            out = super().plan(*a, **k)
            plans.append(out[0])
            return out

    edit = se.MapEdit(Backend())
    n2 = P
    for it in (1, 10, 11):                                   # off the beat (Adam gets its state), the edits, off the beat again
        opt.zero_grad(set_to_none=True)
        pts = params['means3D']
        tp = (w2c @ torch.cat((pts, torch.ones_like(pts[:, :1])), 1).T).T[:, :3]
        im, radius, depth_sil, rv = render_rgb_depth_sil(params, cam, w2c, tp)
        variables['means2D'] = rv['means2D']
        loss = (im - 0.3).abs().sum() + 0.5 * (depth_sil[0] - 2.0).abs().sum()
        loss.backward()
        se.update_seen_and_radius(variables, radius)
        if it == 10:
            rows = int(params['means3D'].shape[0])
            rm = se.prune_mask(params, 0.3, 0.1)
            params, variables = edit.prune_gaussians(params, variables, opt, it, prune_cfg)
            n1 = rows - int(rm.sum())
            assert 0 < int(rm.sum()) < rows and params['means3D'].shape[0] == n1 == plans[-1].n_keep
            assert variables['denom'].shape[0] == n1 == variables['timestep'].shape[0] and variables['seen'].shape[0] == rows
            # the pruned map no longer matches what was rendered: the statistics densify reads are those of the kept rows
            keep = ~rm
            variables['seen'] = variables['seen'][keep]
            grad = rv['means2D'].grad[keep]
            variables['means2D'] = torch.zeros_like(grad).requires_grad_(True)
            variables['means2D'].grad = grad
            v2 = {k: (v.clone() if torch.is_tensor(v) and k != 'means2D' else v) for k, v in variables.items()}
            se.accumulate_mean2d_gradient(v2)
            to_clone, to_split = se.densify_masks(params, v2, 0.0)
            nc, ns = int(to_clone.sum()), int(to_split.sum())
            assert nc > 10 and ns > 10
            params, variables = edit.densify(params, variables, opt, it, dens_cfg)
            stage1, stage2 = plans[-2], plans[-1]
            assert (stage1.n_keep, stage1.n_clone, stage1.n_split) == (n1 - ns, nc, ns) and stage1.rows == n1 - ns + nc + 2 * ns == stage2.P
            n2 = int(params['means3D'].shape[0])
            assert n2 == stage2.n_keep and 0 < n2 <= stage1.rows
            assert not bool(se.prune_mask(params, 0.3, 0.1 * 3.0).any()), "a row that the second stage should have removed is left"
            for k in ('means2D_gradient_accum', 'denom', 'max_2D_radius', 'timestep'):
                assert variables[k].shape[0] == n2 and (k == 'timestep' or not bool(variables[k].any()))
        else:
            params, variables = edit.prune_gaussians(params, variables, opt, it, prune_cfg)    # off the beat: nothing happens
            params, variables = edit.densify(params, variables, opt, it, dens_cfg)              # accumulates only
            assert params['means3D'].shape[0] == n2 and len(plans) == (0 if it == 1 else 3) and float(variables['denom'].sum()) > 0
        opt.step()
        for k, v in params.items():
            assert v.shape[0] == params['means3D'].shape[0] and bool(torch.isfinite(v).all()), k
            s = opt.state.get(v, None)
            # the state made at iteration 1 followed the map through the edits of iteration 10 (whose step saw no gradient)
            assert s and s['exp_avg'].shape == v.shape == s['exp_avg_sq'].shape and bool(torch.isfinite(s['exp_avg']).all()), k
            assert float(s['step']) == (2.0 if it == 11 else 1.0), k
    assert float(opt.state[params['means3D']]['exp_avg'].abs().sum()) > 0


def test_argument_errors_leave_the_library_usable(gpu):
    from fisher_rast import _lib
    lib = _lib.load()
    P = 300
    masks = _masks(P, "random-50")
    rc, st, lists, intact, ws = _plan(gpu, P, masks, short=4)
    assert rc == _lib.FR_ENOSPACE and intact and b"workspace" in lib.fr_last_error()
    assert np.all(ws.get() == GUARD_BITS), "a refused plan wrote to the workspace"
    rc, st, lists, intact, ws = _plan(gpu, P, masks)
    assert rc == 0
    nk, nc, ns = (len(l) for l in lists)
    rows = nk + nc + 2 * ns
    src = torch.arange(P * 16, dtype=torch.int32, device=gpu)
    dst = torch.zeros(rows * 16 + P * 16, dtype=torch.int32, device=gpu)
    A = _lib.MapEditArray

    def call(entries, n=None):
        arr = (A * len(entries))(*entries)
        rc = lib.fr_map_edit_apply(arr, len(entries) if n is None else n, P, nk, nc, ns, 2, ws.ptr, _stream(gpu))
        torch.cuda.synchronize()
        return rc

    good = A(src.data_ptr(), dst.data_ptr(), 3, _lib.FR_EDIT_COPY)
    EINVAL = 1
    assert call([A(src.data_ptr(), src.data_ptr(), 3, 0)]) == EINVAL                                      # in place
    assert call([A(src.data_ptr(), src.data_ptr() + 8, 3, 0)]) == EINVAL                                  # destination inside the source
    assert call([good, A(src.data_ptr(), dst.data_ptr() + 4 * (rows * 3 - 1), 3, 0)]) == EINVAL           # two destinations overlap
    assert call([good, A(dst.data_ptr(), dst.data_ptr() + 4 * rows * 16, 1, 0)]) == EINVAL                # a source that is another's destination
    assert call([A(src.data_ptr(), dst.data_ptr(), 0, 0)]) == EINVAL and call([A(src.data_ptr(), dst.data_ptr(), 17, 0)]) == EINVAL
    assert call([A(src.data_ptr(), dst.data_ptr(), 3, 2)]) == EINVAL                                      # neither COPY nor ZERO
    assert call([good] * 33) == EINVAL and b"FR_EDIT_MAX_ARRAYS" in lib.fr_last_error()
    assert not bool(dst.any()), "a refused call wrote"
    assert lib.fr_map_edit_split_children(4, 2, 2, src.data_ptr(), dst.data_ptr(), src.data_ptr(), dst.data_ptr(), _stream(gpu)) == EINVAL
    # a good call still works
    assert call([good]) == 0
    x = src[:P * 3].reshape(P, 3)
    keep, clone, split = (torch.from_numpy(m).to(gpu) for m in masks)
    want = torch.cat((x[keep], x[clone], x[split].repeat(2, 1)))
    assert torch.equal(dst[:rows * 3].reshape(rows, 3), want) and not bool(dst[rows * 3:].any())
