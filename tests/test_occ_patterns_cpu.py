"""The synthetic occupancy maps of tests/occ_patterns.py have the properties they are named for, checked with a plain flood
fill and shifted-array morphology (no scipy.ndimage), and the CPU restatement (oracle/occupancy_frontier.py) answers on them
what the GPU tests expect.  Keeps the fixtures of tests/test_gpu_occupancy_topology.py honest without a GPU."""
import numpy as np
import pytest

import occ_patterns as op
from occ_patterns import FREE, UNKNOWN

METHODS = ("combined", "largest", "closest")


def _free(name):
    lab, cam = op.cases()[name]
    return lab, cam, (lab == FREE)


@pytest.mark.parametrize("name", ["serpentine", "serpentine_t", "spiral"])
def test_corridor_mazes_are_one_long_chain(name):
    lab, cam, free = _free(name)
    assert lab.shape == (193, 257)
    assert np.array_equal(op.open3(free), free)                       # every free cell survives the opening
    cc, sizes = op.flood_components(free)
    assert len(sizes) == 1 and sizes[0] == free.sum()
    if name != "spiral":
        assert free.sum() == 36861
    # a chain, not a blob: 4-connected too, and cutting one wall gap (a 3-cell link) splits it in two
    assert len(op.flood_components(free, "none")[1]) == 1
    om = op.oracle_map(lab, cam)
    assert np.array_equal(om.build_connected_freespace(None), free.astype(np.uint8))
    # the walk is long: the 4-connected geodesic distance from the first to the last free cell exceeds 10 000 cells
    ys, xs = np.where(free)
    dist = np.full(free.shape, -1, dtype=np.int64)
    dist[ys[0], xs[0]] = 0
    front = [(int(ys[0]), int(xs[0]))]
    while front:
        nxt = []
        for y, x in front:
            for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                yy, xx = y + dy, x + dx
                if 0 <= yy < free.shape[0] and 0 <= xx < free.shape[1] and free[yy, xx] and dist[yy, xx] < 0:
                    dist[yy, xx] = dist[y, x] + 1
                    nxt.append((yy, xx))
        front = nxt
    assert dist.max() > 10_000


@pytest.mark.parametrize("name", ["diagonal", "diagonal_mirror"])
def test_diagonal_chains_hang_on_corner_links(name):
    lab, cam, free = _free(name)
    assert free.sum() == 540 and np.array_equal(op.open3(free), free)
    assert sorted(op.flood_components(free)[1]) == [180, 360]
    n4 = op.flood_components(free, "none")[1]
    assert len(n4) == 60 and (n4 == 9).all()
    want = op.expected_free_space(lab)
    assert want.sum() == 360
    assert np.array_equal(op.oracle_map(lab, cam).build_connected_freespace(None), want)
    # the long chain descends to the right (mirror: to the left): it needs the up-left link (mirror: the up-right link)
    broken, whole = ("anti", "main") if name == "diagonal" else ("main", "anti")
    assert op.flood_components(free, broken)[1].max() == 180
    assert op.flood_components(free, whole)[1].max() == 360


@pytest.mark.parametrize("name,n", [("rectangles2", 2), ("rectangles3", 3)])
def test_equal_rectangles_tie_goes_to_the_first(name, n):
    lab, cam, free = _free(name)
    assert np.array_equal(op.open3(free), free)
    cc, sizes = op.flood_components(free)
    assert len(sizes) == n and (sizes == 84).all()
    got = op.oracle_map(lab, cam).build_connected_freespace(None)
    assert np.array_equal(got, (cc == 1).astype(np.uint8))


def _frontier_facts(name, method):
    lab, cam = op.cases()[name]
    free = op.expected_free_space(lab)
    frontier, cc, sizes, qual = op.frontier_components(lab, free)
    om = op.oracle_map(lab, cam)
    det = {}
    pts, ofree = om.build_frontiers(None, method=method, details=det)
    assert np.array_equal(ofree, free) and np.array_equal(det["frontier"], frontier.astype(np.uint8))
    assert det.get("components", 0) == len(qual)
    return lab, cam, free, frontier, cc, sizes, qual, pts, det


def test_gapped_room_has_a_three_way_tie():
    lab, cam, free, frontier, cc, sizes, qual, pts, det = _frontier_facts("gapped_room", "largest")
    assert frontier.sum() == 18 and list(sizes) == [24, 24, 24] and list(qual) == [1, 2, 3]
    assert np.array_equal(det["target"], (cc == 3).astype(np.uint8)) and len(pts) == 24        # last in raster order: the bottom gap
    assert np.where(cc == 3)[0].min() > np.where(cc == 2)[0].max()
    for method in ("combined", "closest"):
        keys = op.selection_keys(cc, sizes, qual, cam, method)
        assert op.key_gap(keys) > 1e-9
        _, _, _, _, _, _, _, _, d = _frontier_facts("gapped_room", method)
        assert np.array_equal(d["target"], (cc == qual[int(np.argmax(keys))]).astype(np.uint8))


@pytest.mark.parametrize("name", ["perforated", "perforated_full"])
def test_perforated_slab_has_many_components_per_wave(name):
    lab, cam, free, frontier, cc, sizes, qual, pts, det = _frontier_facts(name, "largest")
    assert np.array_equal(free, (lab == FREE).astype(np.uint8))
    islands = int((sizes == 25).sum())
    assert islands > 100 and len(qual) == len(sizes) == islands + (0 if name == "perforated_full" else 1)
    # several distinct components inside one 64-cell segment of a row (one wave of the flatten kernel)
    flat = cc.reshape(-1)
    per_wave = [len(set(flat[i:i + 64]) - {0}) for i in range(0, flat.size, 64)]
    assert max(per_wave) >= 6
    if name == "perforated_full":                                     # all equal: `largest` takes the last in raster order
        assert np.array_equal(det["target"], (cc == len(sizes)).astype(np.uint8))
    for method in ("combined", "closest"):
        assert op.key_gap(op.selection_keys(cc, sizes, qual, cam, method)) > 1e-9


@pytest.mark.parametrize("side", ["top", "bottom", "left", "right"])
def test_border_strips_sit_on_the_min_area_boundary(side):
    for n, dilated in ((3, 10), (4, 12)):
        lab, cam, free, frontier, cc, sizes, qual, pts, det = _frontier_facts(f"strip_{side}_{n}", "combined")
        assert free.sum() == 90 and frontier.sum() == n and list(sizes) == [dilated]
        if n == 3:
            assert len(qual) == 0 and pts is None and "target" not in det
        else:
            assert len(qual) == 1 and len(pts) == 12 and det["target"].sum() == 12
    edge = {"top": lab[0], "bottom": lab[-1], "left": lab[:, 0], "right": lab[:, -1]}[side]
    assert (edge == UNKNOWN).sum() == 4 and (lab == UNKNOWN).sum() == 4


def test_comb_root_is_far_from_its_bulk():
    lab, cam, free = _free("comb")
    assert np.array_equal(op.open3(free), free)
    cc, sizes = op.flood_components(free)
    assert len(sizes) == 2 and sizes[0] == 160 and sizes[1] > 10 * sizes[0]      # the decoy comes first, the comb is larger
    idx = np.where((cc == 2).reshape(-1))[0]
    assert idx[0] // 256 == 257 // 256 and np.median(idx) // 256 - idx[0] // 256 > 100       # workgroups of 256 cells
    assert (cc[1] == 2).sum() == 3                                                      # the root row holds one 3-cell tooth
    assert np.array_equal(op.oracle_map(lab, cam).build_connected_freespace(None), (cc == 2).astype(np.uint8))


@pytest.mark.parametrize("name", sorted(op.cases()))
def test_every_case_has_a_testable_selection(name):
    """`combined` and `closest` compare means of fp64 sums whose order is not fixed on the GPU: the best and the second-best
    key must differ by more than 1e-9 relative on every map (reordering at most 1e5 fp64 terms moves a sum by ~1e-11)."""
    lab, cam = op.cases()[name]
    free = op.expected_free_space(lab)
    frontier, cc, sizes, qual = op.frontier_components(lab, free)
    for method in ("combined", "closest"):
        assert op.key_gap(op.selection_keys(cc, sizes, qual, cam, method)) > 1e-9
    om = op.oracle_map(lab, cam)
    assert np.array_equal(om.build_connected_freespace(None), free)
