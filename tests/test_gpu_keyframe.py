"""-m gpu: the keyframe overlap (fr_keyframe_valid_pixels / fr_keyframe_overlap, csrc/fr_keyframe.hip) and the drop-in written on it
(models/SLAM/utils/keyframe_selection.py).

Through the C ABI on guarded buffers against the g++ harness over the same header: index list, counts, flags and status equal, the
points bit for bit, guards intact, every nullable output null in turn -- at the smallest shapes at which the kernels can still go
wrong (one pixel, ragged workgroups and waves, one point, a tile of 256 keys more or less, the cap, no keyframe, more keyframes than
a wave).  The drop-in on the device against the reference-order torch chain on the CPU, with its two host reads counted."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

import keyframe_cases as kc

pytestmark = pytest.mark.gpu

GUARD = 256                   # bytes behind every buffer
GUARD_BYTE = 0x5A


@pytest.fixture(scope="module")
def kf_harness():
    return kc.build_harness()


class _Guarded:
    """a device buffer of n bytes (8-byte aligned), filled with the guard pattern, with GUARD more bytes behind it"""

    def __init__(self, n, dev):
        self.buf = torch.full((n + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
        self.n = n

    @property
    def ptr(self):
        return self.buf.data_ptr()

    def get(self, dtype):
        return self.buf[:self.n].cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.buf[self.n:] == GUARD_BYTE).all())

    def untouched(self):
        return bool((self.buf == GUARD_BYTE).all())


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _valid_pixels(dev, depth, mask=None):
    """fr_keyframe_valid_pixels on guarded buffers: (idx [count], status [4], every guard intact, the words of idx behind count untouched)"""
    from fisher_rast import _lib
    lib = _lib.load()
    H, W = depth.shape[-2], depth.shape[-1]
    nws = int(lib.fr_keyframe_valid_pixels_workspace_bytes(H, W))
    assert nws > 0
    idx, status, ws = _Guarded(4 * H * W, dev), _Guarded(16, dev), _Guarded(nws, dev)
    d = _dev(depth.astype(np.float32), dev)
    m = None if mask is None else _dev(np.asarray(mask != 0, np.uint8), dev)
    _lib.check(lib.fr_keyframe_valid_pixels(H, W, d.data_ptr(), None if m is None else m.data_ptr(), idx.ptr, status.ptr, ws.ptr, nws, _stream(dev)),
               "fr_keyframe_valid_pixels")
    torch.cuda.synchronize()
    st = status.get(np.int32)
    words = idx.get(np.int32)
    count = int(st[0])
    assert 0 <= count <= H * W
    rest = np.all(words[count:].view(np.uint8) == GUARD_BYTE)
    return words[:count].copy(), st, idx.intact() and status.intact() and ws.intact(), bool(rest)


def _overlap(dev, c, valid_idx="case", draws=None, edge=None, null=(), short_table=False):
    """fr_keyframe_overlap on guarded buffers; `null`: the nullable outputs to leave out.  dict(counts, valid, pts, status, intact)"""
    from fisher_rast import _lib
    lib = _lib.load()
    H, W = c["H"], c["W"]
    vi = c["valid_idx"] if isinstance(valid_idx, str) else valid_idx
    d = np.ascontiguousarray(c["draws"] if draws is None else draws, np.int64)
    n, K = len(d), c["kf_w2c"].shape[0]
    nws = int(lib.fr_keyframe_overlap_workspace_bytes(n))
    assert nws > 0
    out = dict(counts=_Guarded(4 * K, dev), valid=_Guarded(n, dev), pts=_Guarded(12 * n, dev), status=_Guarded(16, dev), ws=_Guarded(nws, dev))
    depth, intr, w2c, kf = _dev(c["depth"], dev), _dev(c["K"], dev), _dev(c["w2c"], dev), _dev(c["kf_w2c"], dev)
    vi_d, d_d = None if vi is None else _dev(np.asarray(vi, np.int32), dev), _dev(d, dev)
    masks = [None if m is None else _dev(np.asarray(np.asarray(m) != 0, np.uint8), dev) for m in c["kf_masks"]]
    table = _dev(np.array([0 if m is None else m.data_ptr() for m in masks], np.uint64).view(np.int64), dev) if any(m is not None for m in masks) else None
    cfg = _lib.KeyframeCfg(H, W, n, K, c["edge"] if edge is None else edge, 0 if vi is None else len(vi), intr.data_ptr(), w2c.data_ptr())
    ptr = lambda k: None if k in null else out[k].ptr
    _lib.check(lib.fr_keyframe_overlap(ctypes.byref(cfg), depth.data_ptr(), None if vi_d is None else vi_d.data_ptr(), d_d.data_ptr(),
                                       kf.data_ptr() if K else None, None if table is None else table.data_ptr(), out["counts"].ptr if K else None,
                                       ptr("valid"), ptr("pts"), out["status"].ptr, out["ws"].ptr, nws, _stream(dev)), "fr_keyframe_overlap")
    torch.cuda.synchronize()
    res = dict(counts=out["counts"].get(np.int32), valid=out["valid"].get(np.uint8), pts=out["pts"].get(np.uint32).reshape(n, 3),
               status=out["status"].get(np.int32), intact=all(g.intact() for g in out.values()))
    for k in null:
        assert out[k].untouched(), (k, "a null output was written")
    return res


def _same(got, want, tag, null=()):
    assert got["intact"], tag
    assert np.array_equal(got["counts"], want["counts"]), (tag, got["counts"], want["counts"])
    assert got["status"].tolist() == want["status"].tolist(), (tag, got["status"], want["status"])
    if "valid" not in null:
        assert np.array_equal(got["valid"], want["valid"]), tag
    if "pts" not in null:
        assert np.array_equal(got["pts"], want["pts"].view(np.uint32)), tag


def _shape_case(H, W, n, K, edge, seed=0):
    """a mixed-mask case at this shape with n draws, however few pixels the frame has"""
    c = kc.make_case("masks-mixed", seed, H, W, n=1, K=K)
    if len(c["valid_idx"]) == 0:
        c["depth"][0, 0, 0] = 1.5
        c["valid_idx"] = kc.np_valid_pixels(c)
    rng = np.random.default_rng([H, W, n, K, seed])
    c["draws"] = rng.integers(0, len(c["valid_idx"]), n).astype(np.int64)
    c["edge"] = edge
    return c


FRAMES = [(1, 1, 0), (1, 1, 2), (5, 7, 0), (5, 7, 2), (48, 64, 0), (48, 64, 2), (63, 65, 0), (63, 65, 2), (256, 256, 20)]


@pytest.mark.parametrize("H,W,edge", FRAMES, ids=[f"{h}x{w}e{e}" for h, w, e in FRAMES])
def test_both_calls_are_the_harness_at_every_frame(gpu, kf_harness, H, W, edge):
    c = _shape_case(H, W, 257 if H == 256 else 65, 2, edge)
    rng = np.random.default_rng(H * W)
    for mask in (None, rng.uniform(size=(H, W)) < 0.4, np.zeros((H, W), bool)):
        want, wst = kc.harness_valid_pixels(kf_harness, c["depth"], mask)
        idx, st, intact, rest = _valid_pixels(gpu, c["depth"], mask)
        assert intact and rest and st.tolist() == wst.tolist() and np.array_equal(idx, want), (H, W, mask is None)
    _same(_overlap(gpu, c), kc.harness_overlap(kf_harness, c), (H, W, edge))
    # a draw is a pixel: no index list
    direct = c["valid_idx"][c["draws"]].astype(np.int64)
    _same(_overlap(gpu, c, valid_idx=None, draws=direct), kc.harness_overlap(kf_harness, c, valid_idx=None, draws=direct), (H, W, edge, "direct"))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1600, 4096])
def test_overlap_at_every_point_count(gpu, kf_harness, n):
    from fisher_rast import _lib
    assert _lib.FR_KEYFRAME_MAX_POINTS == 4096
    c = _shape_case(48, 64, n, 2, 2, seed=n)
    want = kc.harness_overlap(kf_harness, c)
    got = _overlap(gpu, c)
    _same(got, want, n)
    again = _overlap(gpu, c)
    assert all(np.array_equal(got[k], again[k]) for k in ("counts", "valid", "pts", "status")), (n, "second call")
    assert n < 64 or 0 < want["status"][0] < n                     # with replacement: some pixels come twice, some once


@pytest.mark.parametrize("K", [0, 1, 2, 17, 65])
def test_overlap_at_every_keyframe_count(gpu, kf_harness, K):
    c = _shape_case(48, 64, 65, K, 2, seed=K)
    want = kc.harness_overlap(kf_harness, c)
    _same(_overlap(gpu, c), want, K)
    assert K < 2 or want["counts"].any()
    for null in (("valid",), ("pts",), ("valid", "pts")):
        _same(_overlap(gpu, c, null=null), want, (K, null), null)
    # no keyframe carries a mask: a null table
    c["kf_masks"] = [None] * K
    _same(_overlap(gpu, c), kc.harness_overlap(kf_harness, c), (K, "no masks"))


@pytest.mark.parametrize("family", kc.FAMILIES)
def test_every_family_is_the_harness(gpu, kf_harness, family):
    c = kc.make_case(family)
    idx, st, intact, rest = _valid_pixels(gpu, c["depth"], c["curr_mask"])
    assert intact and rest and np.array_equal(idx, c["valid_idx"]) and st.tolist() == [len(idx), 0, 0, 0]
    if len(c["draws"]):
        _same(_overlap(gpu, c), kc.harness_overlap(kf_harness, c), family)


@pytest.mark.parametrize("last", [63, 64, 255, 256, 48 * 64 - 1])
def test_last_valid_pixel_at_a_wave_boundary(gpu, kf_harness, last):
    """the last valid pixel in the last lane of a wave, in the first lane of the next, and the same across two workgroups"""
    depth = np.zeros((1, 48, 64), np.float32)
    depth.reshape(-1)[[0, 5, 62, last]] = 1.0
    idx, st, intact, rest = _valid_pixels(gpu, depth)
    assert intact and rest and idx.tolist() == sorted({0, 5, 62, last}) and st[0] == len(idx)
    depth.reshape(-1)[:last + 1] = 2.0
    idx, st, intact, rest = _valid_pixels(gpu, depth)
    assert intact and rest and np.array_equal(idx, np.arange(last + 1)) and st.tolist() == [last + 1, 0, 0, 0]


def test_out_of_range_draws_and_entries_are_counted_not_read(gpu, kf_harness):
    c = _shape_case(48, 64, 65, 2, 2, seed=3)
    draws = c["draws"].copy()
    draws[7], draws[64] = len(c["valid_idx"]), -1                                  # one past the list, and a negative one
    draws[20] = 1 << 40
    vi = c["valid_idx"].copy()
    vi[draws[9]] = 48 * 64                                                         # an entry one past the frame
    vi[draws[11]] = -5
    want = kc.harness_overlap(kf_harness, c, valid_idx=vi, draws=draws)
    hit = int(np.isin(draws, [draws[9], draws[11]]).sum())
    assert want["status"][1] == 3 + hit and not want["valid"][[7, 9, 11, 20, 64]].any() and not want["pts"][[7, 9, 11, 20, 64]].any()
    _same(_overlap(gpu, c, valid_idx=vi, draws=draws), want, "out of range")
    direct = c["valid_idx"][c["draws"]].astype(np.int64)
    direct[3], direct[4] = 48 * 64, -1
    want = kc.harness_overlap(kf_harness, c, valid_idx=None, draws=direct)
    assert want["status"][1] == 2
    _same(_overlap(gpu, c, valid_idx=None, draws=direct), want, "out of range, direct")


def test_front_end_has_no_host_synchronisation(gpu, kf_harness):
    from fisher_rast import ops
    c = kc.make_case("masks-mixed", 0, 96, 128, n=24, K=5)
    depth, K, w2c = _dev(c["depth"], gpu), _dev(c["K"], gpu), _dev(c["w2c"], gpu)
    kf = _dev(c["kf_w2c"], gpu)
    masks = [None if m is None else _dev(m, gpu) for m in c["kf_masks"]]
    draws = torch.from_numpy(c["draws"])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        idx, status = ops.keyframe_valid_pixels(depth)
        out = ops.keyframe_overlap(depth, K, w2c, draws, kf, valid_idx=idx, n_valid_idx=len(c["valid_idx"]), kf_masks=masks, edge=c["edge"], want_pts=True)
        host = ops.keyframe_overlap(depth, torch.from_numpy(c["K"]), c["w2c"], draws, kf, valid_idx=idx, n_valid_idx=len(c["valid_idx"]), kf_masks=masks, edge=c["edge"])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    want = kc.harness_overlap(kf_harness, c)
    assert int(status[0]) == len(c["valid_idx"]) and np.array_equal(idx[:len(c["valid_idx"])].cpu().numpy(), c["valid_idx"])
    for o in (out, host):
        assert np.array_equal(o["counts"].cpu().numpy(), want["counts"]) and o["status"].cpu().numpy().tolist() == want["status"].tolist()
        assert np.array_equal(o["valid"].cpu().numpy(), want["valid"])
    assert np.array_equal(out["pts"].cpu().numpy().view(np.uint32), want["pts"].view(np.uint32)) and host["pts"] is None


@pytest.mark.parametrize("family", ["generic", "masks-mixed"])
def test_drop_in_on_the_device_against_the_torch_chain(gpu, family):
    """identical lists under the same seeds, k below and above the number of overlapping keyframes; exactly two host reads a call"""
    from models.SLAM.utils import keyframe_selection as ks
    c = None
    for seed in range(kc.MAX_SEEDS):
        cand = kc.make_case(family, seed, 96, 128, n=24 if family.startswith("masks") else 64, K=5)
        cand["edge"] = 20
        if kc.qualifies(cand):
            c = cand
            break
    assert c is not None
    cpu = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    kfs_cpu, kfs_dev = kc.keyframe_list(c), kc.keyframe_list(c, gpu)
    depth, w2c, K = _dev(c["depth"], gpu), _dev(c["w2c"], gpu), _dev(c["K"], gpu)          # uploaded outside the counted stretch
    for k in (2, 9):
        torch.manual_seed(c["seed"]); np.random.seed(5)
        want = kc.torch_chain(cpu(c["depth"]), cpu(c["w2c"]), cpu(c["K"]), kfs_cpu, k, pixels=len(c["draws"]))
        torch.manual_seed(c["seed"]); np.random.seed(5)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("warn")
        try:
            with warnings.catch_warnings(record=True) as w:
                warnings.simplefilter("always")
                got = ks.keyframe_selection_overlap(depth, w2c, K, kfs_dev, k, pixels=len(c["draws"]))
        finally:
            torch.cuda.set_sync_debug_mode("default")
        syncs = [x for x in w if "synchroniz" in str(x.message).lower() and "prototype" not in str(x.message).lower()]
        print(f"k = {k}: selected {got}, host synchronisations {len(syncs)}")
        assert got == want and len(got) == min(k, 5) and len(syncs) == 2, (got, want, [str(x.message) for x in syncs])
    pts = ks.get_pointcloud(depth, K, w2c, torch.tensor([[10, 12], [10, 12], [20, 30]], device=gpu))
    want = kc.torch_pointcloud(cpu(c["depth"]), cpu(c["K"]), cpu(c["w2c"]), torch.tensor([[10, 12], [10, 12], [20, 30]]))
    assert pts.shape == want.shape == (1, 3) and torch.allclose(pts.cpu(), want, rtol=0, atol=1e-5)
