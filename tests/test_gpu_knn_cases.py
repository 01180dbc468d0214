"""-m gpu: fr_knn_dist2 and fr_spatial_order at the edge sizes and on the hard clouds of tests/knn_cases.py (qualified without a
GPU in tests/test_knn_cases_cpu.py).

fr_knn_dist2: `array_equal` on the uint32 views against the brute-force oracle (the same arithmetic in the same order) -- the size
sweep over wave, sub-box, box, sort-chunk and power-of-two edges, one case past the 65536 points that the bounding-box reduction
covers without striding, every family with its closed-form values, metamorphic checks that need no oracle, a workspace that arrives
holding 0x00 or 0xFF, the bytes around the workspace, the output and the input, and the rejections.

fr_spatial_order: the order equals np.argsort(code, kind="stable") of the restated codes -- the size sweep, 0-1 key patterns for the
data-oblivious network, the degenerate and non-finite families, and the empty map."""
import functools

import numpy as np
import pytest
import torch

import knn_cases as kc

pytestmark = pytest.mark.gpu

INF_BITS = 0x7F800000


@functools.lru_cache(maxsize=None)
def _case(family, P, seed=0):
    """the cloud and the oracle's statement of it, computed once and shared (read-only)"""
    from oracle import ref
    ref.build()
    m = kc.make_cloud(family, P, seed)
    want = ref.knn_dist2(m)
    for a in (m, want):
        a.setflags(write=False)
    return m, want


def _dev(a, gpu):
    return torch.from_numpy(np.array(a)).to(gpu)             # (a copy: the shared cases are read-only)


def _knn(m, gpu):
    from fisher_rast.ops import knn_dist2
    return knn_dist2(_dev(m, gpu)).cpu().numpy()


def _same_bits(got, want, what):
    got, want = kc.bits(got), kc.bits(want)
    assert got.shape == want.shape, what
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (what, f"{diff.size} rows differ, first {diff[:8].tolist()}")


# ---- fr_knn_dist2 against the oracle ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("P", kc.KNN_SWEEP)
@pytest.mark.parametrize("family", ["uniform", "clusters"])
def test_knn_size_sweep(gpu, family, P):
    m, want = _case(family, P)
    got = _knn(m, gpu)
    _same_bits(got, want, (family, P))
    if P < 4:
        assert (kc.bits(got) == INF_BITS).all()               # fewer than three neighbours: FLT_MAX stays in the sum
    else:
        assert np.isfinite(got).all()


def test_knn_one_point_past_the_grid_cap(gpu):
    """65537 points: the 256 workgroups of the bounding-box reduction stride, and the network has one key past a power of two"""
    m, want = _case("uniform", kc.KNN_PAST_THE_GRID_CAP)
    _same_bits(_knn(m, gpu), want, "uniform 65537")


@pytest.mark.parametrize("family,P", [(f, P) for f, sizes in kc.KNN_FAMILY_SIZES.items() for P in sizes])
def test_knn_families(gpu, family, P):
    m, want = _case(family, P)
    got = _knn(m, gpu)
    _same_bits(got, want, (family, P))
    if family == "lattice":
        _same_bits(got, np.full(P, kc.LATTICE_ANSWER), "0.0625 everywhere, corners included")
    elif family == "point":
        assert not kc.bits(got).any()
    elif family == "dup_groups":
        for g in kc.dup_group_rows(P):
            assert (got[g] > 0).all() if len(g) <= 3 else not kc.bits(got[g]).any(), (len(g), got[g])
    elif family == "nonfinite":
        bad = ~np.isfinite(m).all(1)
        assert (kc.bits(got[bad]) == INF_BITS).all()
        _same_bits(_knn(m[~bad], gpu), got[~bad], "the cloud with the non-finite rows deleted")
    elif family == "overflow":
        assert (kc.bits(got) == INF_BITS).all()


# ---- metamorphic: no oracle ---------------------------------------------------------------------------------------------------------------

def test_knn_permuted_rows_give_the_permuted_result(gpu):
    m = kc.metamorphic_cloud()
    perm = np.random.default_rng(11).permutation(len(m))
    _same_bits(_knn(m[perm], gpu), _knn(m, gpu)[perm], "permutation")


@pytest.mark.parametrize("e", [50, -50])
def test_knn_scales_by_an_exact_power_of_two(gpu, e):
    """the cloud times 2^e gives the result times 2^2e bit for bit (the cloud is qualified for it: test_scaling_law_of_the_oracle)"""
    m = kc.metamorphic_cloud()
    base = _knn(m, gpu)
    assert (base > 0).any() and (base == 0).sum() >= 50
    _same_bits(_knn(kc.scaled(m, e), gpu), kc.scaled(base, 2 * e), f"2^{e}")


def test_knn_twice_gives_the_same_bits(gpu):
    from fisher_rast.ops import knn_dist2
    d = _dev(kc.metamorphic_cloud(), gpu)
    a = knn_dist2(d).cpu().numpy()
    b = knn_dist2(d).cpu().numpy()
    _same_bits(a, b, "two calls in a row")


# ---- the C entry point: workspace contents, bounds, rejections ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from fisher_rast import _lib
    return _lib.load()


def _raw(lib, P, points, out, ws, nbytes):
    """fr_knn_dist2 on the null stream (the tensors were filled on it), then a synchronise"""
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = lib.fr_knn_dist2(P, ptr(points), ptr(out), ptr(ws), nbytes, None)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("fill", [0x00, 0xFF])
@pytest.mark.parametrize("family,P", [("clusters", 2049), ("seam", 4097)])
def test_knn_stale_workspace(gpu, lib, family, P, fill):
    """callers hand over torch.empty: whatever the workspace held before must not reach the result"""
    m, want = _case(family, P)
    pts = _dev(m, gpu)
    nbytes = int(lib.fr_knn_workspace_bytes(P))
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=gpu)
    out = torch.full((P,), float("nan"), device=gpu)
    assert _raw(lib, P, pts, out, ws, nbytes) == 0
    _same_bits(out.cpu().numpy(), want, (family, P, hex(fill)))


@pytest.mark.parametrize("P", [1, 64, 65, 1025, 2049])
def test_knn_writes_nothing_out_of_range(gpu, lib, P):
    """workspace_bytes exactly fr_knn_workspace_bytes(P) inside a larger allocation, `out` inside a longer tensor: the 4 KiB behind
    the workspace, the head and the tail around `out` and the input points are unchanged, and the result is the oracle's"""
    m, want = _case("clusters", P)
    pts = _dev(m, gpu)
    nbytes = int(lib.fr_knn_workspace_bytes(P))
    tail = (torch.arange(4096, device=gpu) % 251).to(torch.uint8)
    ws = torch.cat([torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=gpu), tail])
    pad = 64
    pattern = (torch.arange(P + 2 * pad, device=gpu, dtype=torch.int32) * 7919 + 0x5A5A0000).view(torch.float32)
    buf = pattern.clone()
    out = buf[pad:pad + P]
    assert _raw(lib, P, pts, out, ws, nbytes) == 0
    assert torch.equal(ws[nbytes:], tail)
    as_int = lambda t: t.view(torch.int32)
    assert torch.equal(as_int(buf[:pad]), as_int(pattern[:pad])) and torch.equal(as_int(buf[pad + P:]), as_int(pattern[pad + P:]))
    assert np.array_equal(kc.bits(pts.cpu().numpy()), kc.bits(m))
    _same_bits(out.cpu().numpy(), want, P)


def test_knn_rejections(gpu, lib):
    from fisher_rast import _lib
    P = 1025
    m, _ = _case("clusters", P)
    pts = _dev(m, gpu)
    nbytes = int(lib.fr_knn_workspace_bytes(P))
    ws = torch.zeros((nbytes,), dtype=torch.uint8, device=gpu)
    pattern = (torch.arange(P, device=gpu, dtype=torch.int32) * 7919 + 0x5A5A0000).view(torch.float32)
    out = pattern.clone()
    assert _raw(lib, P, pts, out, ws, nbytes - 1) == _lib.FR_ENOSPACE and b"fr_knn_dist2" in lib.fr_last_error()
    assert _raw(lib, P, pts, None, ws, nbytes) == _lib.FR_EINVAL
    assert _raw(lib, P, None, out, ws, nbytes) == _lib.FR_EINVAL
    assert torch.equal(out.view(torch.int32), pattern.view(torch.int32))          # untouched by all three
    assert not ws.any()


# ---- fr_spatial_order -------------------------------------------------------------------------------------------------------------------

def _check_order(m, gpu, what):
    """a permutation, a stable sort of the restated codes, and exactly np.argsort(code, kind="stable")"""
    from fisher_rast.ops import spatial_order_of
    P = len(m)
    t = spatial_order_of(_dev(m, gpu))
    assert t.dtype == torch.int32 and tuple(t.shape) == (P,)
    order = t.cpu().numpy().astype(np.int64)
    assert np.array_equal(np.sort(order), np.arange(P)), what
    code = kc.morton_np(m)
    c = code[order]
    assert np.all(c[1:] >= c[:-1]), what
    same = c[1:] == c[:-1]
    assert np.all(order[1:][same] > order[:-1][same]), what
    assert np.array_equal(order, np.argsort(code, kind="stable")), what
    return order


@pytest.mark.parametrize("P", kc.ORDER_SWEEP)
def test_order_size_sweep(gpu, P):
    _check_order(kc.make_cloud("uniform", P), gpu, P)


def test_order_frame_set_by_the_point_past_the_grid_cap(gpu):
    """row 65536 alone sets the upper corner of the frame: a bounding-box reduction that did not stride would quantise every point
    on another grid"""
    m = kc.make_cloud("uniform", kc.KNN_PAST_THE_GRID_CAP)
    m[-1] = 3.0
    assert (m[:-1] < 2.0).all()
    _check_order(m, gpu, "corner in the last row")


@pytest.mark.parametrize("P", kc.PATTERN_SIZES)
@pytest.mark.parametrize("pattern", kc.PATTERNS)
def test_order_key_patterns(gpu, pattern, P):
    """the network is data-oblivious, so a wrong comparator shows on 0-1 keys"""
    order = _check_order(kc.pattern_points(pattern, P), gpu, (pattern, P))
    if pattern == "equal":
        assert np.array_equal(order, np.arange(P))
    elif pattern == "descending":
        assert np.array_equal(order, np.arange(P)[::-1])


@pytest.mark.parametrize("family,P", [(f, P) for f, sizes in kc.ORDER_FAMILY_SIZES.items() if f != "nonfinite" for P in sizes])
def test_order_degenerate_families(gpu, family, P):
    order = _check_order(kc.make_cloud(family, P), gpu, (family, P))
    if family == "point":
        assert np.array_equal(order, np.arange(P))            # all keys equal


@pytest.mark.parametrize("kinds", [(np.nan, np.inf, -np.inf), (np.nan,)], ids=["nan-and-inf", "nan-only"])
@pytest.mark.parametrize("P", kc.ORDER_FAMILY_SIZES["nonfinite"])
def test_order_nonfinite(gpu, P, kinds):
    """The restatement follows what k_knn_minmax and k_knn_morton do: the bounds come from fminf / fmaxf, which ignore NaN, and a NaN
    quotient -- a NaN coordinate, inf / inf, inf - inf -- leaves fminf(fmaxf(u, 0), 1) as 0.  With an infinity on an axis its extent
    is infinite and every point's cell on it is 0 (so the full family sorts into index order); with NaN only, the bounds are those
    of the finite coordinates and the NaN coordinates sit in cell 0.  Kernel and restatement agree; neither had to give way."""
    m = kc.make_cloud("nonfinite", P, kinds=kinds)
    order = _check_order(m, gpu, (P, kinds))
    if len(kinds) == 3:
        assert np.array_equal(order, np.arange(P))


def test_order_of_an_empty_map(gpu):
    from fisher_rast.ops import spatial_order_of
    order = spatial_order_of(torch.zeros((0, 3), device=gpu))
    assert order.dtype == torch.int32 and tuple(order.shape) == (0,) and order.device.type == "cuda"
