"""-m gpu: the sort stage of fixed key segments as wave-sized work items.  k_sort_split cuts every long list (2049 .. tile_capacity / 2
- 64 keys) at sampled pivots into parts behind the list and enters each part of 2 .. 512 keys in the PART LIST of the workspace;
k_sort_parts lets any wave sort any part.  The tests read the workspace back and REPLAY the partition on the host (the sample is
taken by position in the unsorted list, which still stands at the start of its segment), so the part list is checked entry by entry,
not in bulk.  No test provokes a fault; the driver gives every GPU step its own time limit."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SMALL_MAX = 2048           # lists up to this many keys are sorted whole (k_sort_tiles' body)


def _part_max(capacity):
    return min(capacity // 2 - 64, 16320)


def _scorer(args, cam, capacity):
    from fisher_rast.ops import FisherScorer
    return FisherScorer(cam, *args, tile_capacity=capacity)


def _cam(W, H, gpu):
    from fisher_rast.synthetic import intrinsics
    from models.SLAM.utils.recon_helpers import setup_camera
    return setup_camera(W, H, intrinsics(W, H), np.eye(4), device=gpu)


def _args(gpu, means, z, rng, opacity=(0.005, 0.02)):
    P = len(z)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return (t(means.astype(np.float32)), t(rng.uniform(0, 1, (P, 3)).astype(np.float32)), t(np.tile(np.array([[1, 0, 0, 0]], np.float32), (P, 1))),
            t(rng.uniform(opacity[0], opacity[1], P).astype(np.float32)), t(np.full((P, 3), 0.004, np.float32) * z[:, None].astype(np.float32)))


def _clustered_depths(rng, n):
    """three 'walls': two tight depth clusters and a uniform spread (the long-list scene of test_gpu_tile_segments.py)"""
    return np.concatenate([rng.normal(2.0, 0.004, n // 3), rng.normal(3.5, 0.004, n // 3), rng.uniform(1.0, 6.0, n - 2 * (n // 3))]).astype(np.float32)


def _one_tile_scene(gpu, P, seed):
    """One tile of a 48 x 48 view takes every splat: a list of exactly P keys per view (asserted by the callers); a quarter of the
    splats are exact duplicates (runs of equal depth, split by the slot)."""
    rng = np.random.default_rng(seed)
    W = H = 48
    z = _clustered_depths(rng, P)
    u = rng.uniform(21.0, 27.0, P); v = rng.uniform(21.0, 27.0, P)
    means = np.stack([(u - 24.0) / 24.0 * z, (v - 24.0) / 24.0 * z, z], 1).astype(np.float32)
    means[P // 2:P // 2 + P // 4] = means[:P // 4]
    z[P // 2:P // 2 + P // 4] = z[:P // 4]
    return W, H, _args(gpu, means, z, rng, opacity=(0.3, 0.6))


def _many_lists_scene(gpu, seed, heavy_lo=2100, heavy_hi=6000, extra=(), all_heavy=False):
    """128 x 128 (8 x 8 tiles): the tiles of one colour of a checkerboard plus a few more are HEAVY (heavy_lo .. heavy_hi splats, clustered
    depths, exact duplicates), the others hold 0 .. 1500.  Splats sit within 3.5 pixels of their tile's centre and are a pixel wide,
    so a list is its tile's own splats under every pose used here.  `extra`: (tile, splats) pairs set by hand; `all_heavy`: no light tile."""
    rng = np.random.default_rng(seed)
    W = H = 128
    per_tile = []
    for ty in range(8):
        for tx in range(8):
            heavy = all_heavy or (tx + ty) % 2 == 0 or (tx % 4 == 1 and ty % 3 == 0)
            per_tile.append(int(rng.integers(heavy_lo, heavy_hi)) if heavy else int(rng.choice([0, 1, 2, 60, 300, 700, 1500])))
    for tile, n in extra:
        per_tile[tile] = n
    zs, us, vs = [], [], []
    for i, n in enumerate(per_tile):
        if n == 0:
            continue
        z = _clustered_depths(rng, n) if n >= 9 else rng.uniform(1.0, 6.0, n).astype(np.float32)
        u = 16.0 * (i % 8) + 8.0 + rng.uniform(-3.5, 3.5, n); v = 16.0 * (i // 8) + 8.0 + rng.uniform(-3.5, 3.5, n)
        if n >= 8:                                                # duplicates inside the tile
            q = n // 4
            z[n // 2:n // 2 + q] = z[:q]; u[n // 2:n // 2 + q] = u[:q]; v[n // 2:n // 2 + q] = v[:q]
        zs.append(z); us.append(u); vs.append(v)
    z, u, v = np.concatenate(zs), np.concatenate(us), np.concatenate(vs)
    means = np.stack([(u - 64.0) / 64.0 * z, (v - 64.0) / 64.0 * z, z], 1).astype(np.float32)
    return W, H, _args(gpu, means, z, rng, opacity=(0.02, 0.2))


def _poses(gpu, V, step=0.004):
    w2c = torch.eye(4, device=gpu)[None].repeat(V, 1, 1)
    for i in range(V):
        w2c[i, 0, 3] = step * (i % 3 - 1); w2c[i, 1, 3] = step * (i // 3 % 3 - 1)
    return w2c


def _read_back(sc, P, W, H, V):
    """tile counts, tile offsets, the key buffer and the part list {count, descriptors [count, 2]} of the scorer's last launch"""
    from fisher_rast import _lib
    lib = _lib.load()
    T = ((W + 15) // 16) * ((H + 15) // 16)
    cap = V * sc._keys_per_view()
    off = (ctypes.c_size_t * 8)()
    _lib.check(lib.fr_fisher_workspace_layout(P, W, H, V, cap, 4, off), "layout")
    po = ctypes.c_size_t(0)
    _lib.check(lib.fr_fisher_part_list_offset(P, W, H, V, cap, 4, ctypes.byref(po)), "part list offset")
    torch.cuda.synchronize()
    ws = sc._ws[0]
    cnt = ws[off[0]:off[0] + V * T * 4].view(torch.int32).cpu().numpy().astype(np.int64)
    toff = ws[off[1]:off[1] + V * T * 4].view(torch.int32).cpu().numpy().astype(np.int64) & 0xffffffff
    keys = ws[off[2]:off[2] + cap * 8].view(torch.int64).cpu().numpy().view(np.uint64)
    head = ws[po.value:po.value + 64].view(torch.int32).cpu().numpy().astype(np.int64) & 0xffffffff
    n_parts = int(head[0])
    assert n_parts <= 64 * V * T, n_parts                          # the region's size
    desc = ws[po.value + 64:po.value + 64 + n_parts * 8].view(torch.int32).cpu().numpy().astype(np.int64).reshape(-1, 2) & 0xffffffff
    return cnt, toff, keys, n_parts, desc


def _replay_partition(unsorted):
    """The parts k_sort_split makes of a list (part sizes in key order): 512 keys sampled by position, sorted; NP - 1 of them are the
    pivots; a key's part is the number of pivots <= it."""
    n = len(unsorted)
    NP = 4 if n <= 1280 else 8 if n <= 2560 else 16 if n <= 5120 else 32 if n <= 10240 else 64
    sample = np.sort(unsorted[(np.arange(512, dtype=np.int64) * n) >> 9])
    piv = sample[(np.arange(1, NP) * 512) // NP]
    return np.bincount(np.searchsorted(piv, unsorted, side="right"), minlength=NP).astype(np.int64)


def _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity):
    """Every segment sorted, a permutation of the unsorted list, moved iff partitioned; the part list EXACTLY the replayed partition's
    parts of 2 .. 512 keys.  Returns (long lists, parts beyond 512 keys, keys no descriptor covers)."""
    want = set()
    n_long = n_over = uncovered = 0
    for i in range(len(cnt)):
        n = int(cnt[i])
        seg = keys[toff[i]:toff[i] + n]
        assert np.all(seg[1:] > seg[:-1]), (i, n)
        parted = SMALL_MAX < n <= _part_max(capacity)
        assert (toff[i] != i * capacity) == parted, (i, n, toff[i])
        if not parted:
            continue
        n_long += 1
        assert toff[i] == i * capacity + ((n + 63) & ~63)
        unsorted = keys[i * capacity:i * capacity + n]
        assert np.array_equal(np.sort(unsorted), seg), (i, n)
        sizes = _replay_partition(unsorted)
        start = toff[i] + np.concatenate([[0], np.cumsum(sizes)[:-1]])
        for o, c in zip(start, sizes):
            if 2 <= c <= 512:
                want.add((int(o), int(c)))
            else:
                uncovered += int(c); n_over += int(c > 512)
    got = [(int(o), int(c)) for o, c in desc]
    assert len(got) == n_parts == len(set(got)), (len(got), n_parts)            # no slot claimed twice, none left unwritten (a repeat or a stale entry)
    assert set(got) == want, (len(want), len(got), sorted(want ^ set(got))[:8])
    # what the rule above implies, stated on the descriptors themselves: ranges of at most 512 keys inside a long list's sorted copy, disjoint
    ordered = sorted(got)
    assert all(2 <= c <= 512 for _, c in ordered)
    assert all(a[0] + a[1] <= b[0] for a, b in zip(ordered, ordered[1:]))
    return n_long, n_over, uncovered


def test_many_long_lists_at_once(gpu):
    """A few hundred long lists in one call, short lists between them: a part-list slot claimed twice, or a stride that skips parts,
    leaves a segment unsorted or a descriptor missing."""
    V, capacity = 8, 16384
    W, H, args = _many_lists_scene(gpu, seed=11)
    P = args[0].shape[0]
    cam = _cam(W, H, gpu)
    w2c = _poses(gpu, V)
    Hi = (torch.rand((P, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    fixed, packed = _scorer(args, cam, capacity), _scorer(args, cam, 0)
    a, b = fixed.run(w2c, H_inv=Hi), packed.run(w2c, H_inv=Hi)
    assert fixed.tile_capacity == capacity
    assert torch.equal(a["num_rendered"], b["num_rendered"]) and torch.equal(a["vis_count"], b["vis_count"])
    assert torch.equal(a["scores"], b["scores"]) and float(a["scores"].min()) > 0
    cnt, toff, keys, n_parts, desc = _read_back(fixed, P, W, H, V)
    n_long, _, uncovered = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)
    n_short = int(((cnt >= 2) & (cnt <= SMALL_MAX)).sum())
    print(f"lists: {n_long} long, {n_short} short, {int((cnt < 2).sum())} trivial; {n_parts} parts, {uncovered} keys in no descriptor")
    assert n_long >= 200 and n_short >= 100
    assert n_parts >= 8 * n_long - 8


@pytest.mark.parametrize("n,capacity", [(2049, 32768), (2560, 32768), (2561, 32768), (5120, 32768), (5121, 32768), (10240, 32768), (10241, 32768),
                                        (16320, 32768), (8128, 16384), (8129, 16384)])
def test_sizes_where_the_part_count_changes_hands(gpu, n, capacity):
    """List lengths at the edges of NP = 8 / 16 / 32 / 64 and of the partitioned range (8129 keys at capacity 16384 is the 1024-thread tier's)."""
    V = 2
    W, H, args = _one_tile_scene(gpu, n, seed=n)
    cam = _cam(W, H, gpu)
    w2c = _poses(gpu, V, step=0.002)
    Hi = (torch.rand((n, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    fixed, packed = _scorer(args, cam, capacity), _scorer(args, cam, 0)
    a, b = fixed.run(w2c, H_inv=Hi), packed.run(w2c, H_inv=Hi)
    assert fixed.tile_capacity == capacity
    assert torch.equal(a["num_rendered"], b["num_rendered"]) and torch.equal(a["scores"], b["scores"]) and float(a["scores"].min()) > 0
    cnt, toff, keys, n_parts, desc = _read_back(fixed, n, W, H, V)
    assert int(cnt.max()) == n and int((cnt == n).sum()) == V, cnt          # the scene's premise: the list length under test
    n_long, n_over, _ = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)
    assert n_long == (V if n <= _part_max(capacity) else 0)
    if n_long == 0:
        assert n_parts == 0


def test_parts_beyond_one_wave(gpu):
    """A part that sampling leaves beyond 512 keys is sorted by the splitting workgroup itself and gets no descriptor.  With NP = 64 a
    part holds 8 of the 512 samples, so at 16000 .. 16320 keys (250 .. 255 expected per part) a part of twice the expected size is a
    one-in-a-hundred event per part (the tail of a Gamma(8) variable beyond 16), about one list in three.  Every tile of the view holds
    such a list, each drawn on its own, so that some of the 128 lists have one whatever order the front end left the keys in; how
    many is read from the replayed partition and asserted."""
    V, capacity = 2, 32768
    W, H, args = _many_lists_scene(gpu, seed=21, heavy_lo=16000, heavy_hi=16321, all_heavy=True)
    P = args[0].shape[0]
    cam = _cam(W, H, gpu)
    w2c = _poses(gpu, V, step=0.002)
    Hi = (torch.rand((P, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    fixed, packed = _scorer(args, cam, capacity), _scorer(args, cam, 0)
    a, b = fixed.run(w2c, H_inv=Hi), packed.run(w2c, H_inv=Hi)
    assert fixed.tile_capacity == capacity
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["num_rendered"], b["num_rendered"]) and float(a["scores"].min()) > 0
    cnt, toff, keys, n_parts, desc = _read_back(fixed, P, W, H, V)
    n_long, n_over, uncovered = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)
    print(f"{n_over} parts beyond 512 keys in {n_long} lists of {int(cnt.min())} .. {int(cnt.max())} keys, {uncovered} keys in no descriptor")
    assert n_long == 64 * V and n_over >= 1


def test_the_part_list_does_not_leak_between_calls(gpu):
    """Two run() calls with different poses, then a launch whose longest list overflows its segment (nothing is sorted, no part is
    listed, no offset moves), then run(), which grows the segments and repeats: every part list is its own call's."""
    V, capacity = 8, 8192
    W, H, args = _many_lists_scene(gpu, seed=12, heavy_lo=2100, heavy_hi=3900)
    P = args[0].shape[0]
    cam = _cam(W, H, gpu)
    Hi = (torch.rand((P, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    fixed, packed = _scorer(args, cam, capacity), _scorer(args, cam, 0)
    seen = []
    for w2c in (_poses(gpu, V), _poses(gpu, V, step=-0.007)[:6]):
        a, b = fixed.run(w2c, H_inv=Hi), packed.run(w2c, H_inv=Hi)
        assert fixed.tile_capacity == capacity and torch.equal(a["scores"], b["scores"])
        cnt, toff, keys, n_parts, desc = _read_back(fixed, P, W, H, len(w2c))
        n_long, _, _ = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)
        assert n_long >= 100
        seen.append(n_parts)
    assert seen[0] != seen[1]
    # one tile beyond its segment
    W, H, args2 = _many_lists_scene(gpu, seed=12, heavy_lo=2100, heavy_hi=3900, extra=((27, 9000),))
    P2 = args2[0].shape[0]
    Hi2 = (torch.rand((P2, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    over, packed2 = _scorer(args2, cam, capacity), _scorer(args2, cam, 0)
    w2c = _poses(gpu, V)
    r = over.launch(w2c, H_inv=Hi2)
    st = r["status"].cpu().numpy()
    assert st[1] == 1 and st[3] == 1 and st[2] > capacity
    cnt, toff, keys, n_parts, desc = _read_back(over, P2, W, H, V)
    assert n_parts == 0 and int((cnt > SMALL_MAX).sum()) >= 100
    assert np.array_equal(toff, np.arange(len(toff), dtype=np.int64) * capacity)               # nothing moved
    got = over.run(w2c, H_inv=Hi2)                                                              # grows the segments, repeats
    assert over.tile_capacity >= int(st[2]) and over.tile_capacity % 1024 == 0
    want = packed2.run(w2c, H_inv=Hi2)
    assert torch.equal(got["scores"], want["scores"]) and torch.equal(got["num_rendered"], want["num_rendered"])
    cnt, toff, keys, n_parts, desc = _read_back(over, P2, W, H, V)
    n_long, _, _ = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, over.tile_capacity)
    assert n_long >= 100 and int(cnt.max()) == int(st[2])


def test_one_view(gpu):
    """V = 1: no fork anywhere in the stage, the split and the parts run on the caller's stream like every other view count."""
    capacity = 16384
    W, H, args = _many_lists_scene(gpu, seed=13)
    P = args[0].shape[0]
    cam = _cam(W, H, gpu)
    w2c = _poses(gpu, 1)
    Hi = (torch.rand((P, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    fixed, packed = _scorer(args, cam, capacity), _scorer(args, cam, 0)
    a, b = fixed.run(w2c, H_inv=Hi), packed.run(w2c, H_inv=Hi)
    assert fixed.tile_capacity == capacity
    assert torch.equal(a["scores"], b["scores"]) and torch.equal(a["num_rendered"], b["num_rendered"]) and float(a["scores"].min()) > 0
    cnt, toff, keys, n_parts, desc = _read_back(fixed, P, W, H, 1)
    n_long, _, _ = _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)
    assert n_long >= 25
