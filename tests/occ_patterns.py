"""Synthetic occupancy maps for the planner-side kernels (csrc/fisher_occ.hip): label images with values
0 unknown, 1 occupied, 2 free, shaped (grid_h, grid_w), built to put the connected-component, selection and compaction
kernels where a map grown from depth views of one convex room never does.  Every free structure is at least 3 cells thick, so
it survives the 3 x 3 opening of build_connected_freespace.  Helper module of tests/test_occ_patterns_cpu.py (which checks,
without scipy.ndimage.label, that each generator has the property it is named for) and tests/test_gpu_occupancy_topology.py.
"""
import numpy as np

UNKNOWN, OCCUPIED, FREE = 0, 1, 2


def onehot(label):
    """(3, gh, gw) float32 map whose arg-max is `label`."""
    label = np.asarray(label)
    occ = np.zeros((3,) + label.shape, dtype=np.float32)
    for l in range(3):
        occ[l][label == l] = 1.0
    return occ


def oracle_map(label, cam_pos, intrinsics=None, cell_size=0.05, map_center=(0.0, 0.0), height_range=(-0.6, 0.6), far=10.0):
    """The CPU restatement (oracle/occupancy_frontier.py) holding `label` as a one-hot map, camera cell (row, col) = cam_pos."""
    from oracle.occupancy_frontier import OccupancyMap
    gh, gw = np.asarray(label).shape
    om = OccupancyMap(np.eye(3) if intrinsics is None else intrinsics, grid_dim=(gw, gh), cell_size=cell_size, map_center=map_center,
                      height_range=height_range, pcd_far_distance=far)
    om.occ_map = onehot(label)
    om.cam_pos = np.array([int(cam_pos[0]), int(cam_pos[1])])
    return om


# ---- corridor mazes: 3-cell corridors, 1-cell occupied walls, one component through one long chain ----------------------
def _corridors(gh, gw, path):
    """`path` walks the coarse grid of 3 x 3 blocks on a pitch of 4 (block (i, j) = rows 1+4i..3+4i, cols 1+4j..3+4j);
    consecutive blocks are joined through the wall between them, all other walls stay."""
    lab = np.full((gh, gw), OCCUPIED, dtype=np.uint8)
    for (i, j) in path:
        lab[1 + 4 * i:4 + 4 * i, 1 + 4 * j:4 + 4 * j] = FREE
    for (i0, j0), (i1, j1) in zip(path[:-1], path[1:]):
        assert abs(i0 - i1) + abs(j0 - j1) == 1
        if i0 == i1:
            lab[1 + 4 * i0:4 + 4 * i0, 4 * max(j0, j1)] = FREE
        else:
            lab[4 * max(i0, i1), 1 + 4 * j0:4 + 4 * j0] = FREE
    return lab


def serpentine(gh, gw):
    """Full-width corridors joined alternately at the right and left ends."""
    ni, nj = (gh - 1) // 4, (gw - 1) // 4
    path = [(i, j if i % 2 == 0 else nj - 1 - j) for i in range(ni) for j in range(nj)]
    return _corridors(gh, gw, path)


def serpentine_t(gh, gw):
    """The transpose: full-height corridors joined at the bottom and top."""
    return np.ascontiguousarray(serpentine(gw, gh).T)


def spiral(gh, gw):
    """Rectangular spiral from the top-left corner inwards."""
    ni, nj = (gh - 1) // 4, (gw - 1) // 4
    top, bot, left, right = 0, ni - 1, 0, nj - 1
    path = []
    while top <= bot and left <= right:
        path += [(top, j) for j in range(left, right + 1)]
        path += [(i, right) for i in range(top + 1, bot + 1)]
        if top < bot:
            path += [(bot, j) for j in range(right - 1, left - 1, -1)]
        if left < right and top < bot:
            path += [(i, left) for i in range(bot - 1, top, -1)]
        top, bot, left, right = top + 1, bot - 1, left + 1, right - 1      # ring k ends one block from ring k + 1's start
    return _corridors(gh, gw, path)


# ---- corner-to-corner chains ------------------------------------------------------------------------------------------
def diagonal_chains(gh, gw, n_long=40, n_short=20, mirror=False):
    """3 x 3 free blocks on an unknown background touching only at corners: n_long blocks descending to the right from the
    top-left, n_short descending to the left from the top-right; the chains do not touch.  mirror flips left and right, so the
    long chain hangs on the other diagonal link."""
    assert 3 * n_long + 3 * n_short + 4 <= gw and 3 * n_long + 2 <= gh
    lab = np.full((gh, gw), UNKNOWN, dtype=np.uint8)
    for k in range(n_long):
        lab[1 + 3 * k:4 + 3 * k, 1 + 3 * k:4 + 3 * k] = FREE
    for k in range(n_short):
        lab[1 + 3 * k:4 + 3 * k, gw - 4 - 3 * k:gw - 1 - 3 * k] = FREE
    return np.ascontiguousarray(lab[:, ::-1]) if mirror else lab


# ---- ties ---------------------------------------------------------------------------------------------------------------
def equal_rectangles(gh, gw, n=2):
    """n disjoint free 12 x 7 rectangles (rows x cols) of identical area on an unknown background, none first in more than
    raster order: later ones sit lower and further left."""
    lab = np.full((gh, gw), UNKNOWN, dtype=np.uint8)
    for k in range(n):
        r, c = 5 + 20 * k, gw - 20 - 31 * k
        lab[r:r + 12, c:c + 7] = FREE
    return lab


def gapped_room(gh, gw, room_w=50, room_h=80, gap=6):
    """A free room behind a 1-cell occupied wall on an unknown background; the wall is unknown along `gap` cells in three
    places (top, left, bottom), which gives three frontier components of equal size after dilation."""
    lab = np.full((gh, gw), UNKNOWN, dtype=np.uint8)
    r0, c0 = (gh - room_h) // 2, (gw - room_w) // 2
    lab[r0:r0 + room_h, c0:c0 + room_w] = OCCUPIED
    lab[r0 + 1:r0 + room_h - 1, c0 + 1:c0 + room_w - 1] = FREE
    lab[r0, c0 + 11:c0 + 11 + gap] = UNKNOWN                         # top wall
    lab[r0 + 30:r0 + 30 + gap, c0] = UNKNOWN                         # left wall
    lab[r0 + room_h - 1, c0 + 27:c0 + 27 + gap] = UNKNOWN            # bottom wall: last in raster order
    return lab


def perforated_slab(gh, gw, full=False):
    """A free slab perforated by 3 x 3 unknown islands on a pitch of 8: every island is a frontier component of 25 cells after
    dilation, several of them in each 64-cell row segment.  full=False leaves an unknown margin of 4 cells round the slab
    (one more, large, frontier component); full=True lets the slab fill the map, so that all components are equal."""
    lab = np.full((gh, gw), UNKNOWN, dtype=np.uint8)
    m = 0 if full else 4
    lab[m:gh - m, m:gw - m] = FREE
    for r in range(m + 4, gh - m - 6, 8):
        for c in range(m + 4, gw - m - 6, 8):
            lab[r:r + 3, c:c + 3] = UNKNOWN
    return lab


# ---- the size > min_area boundary ---------------------------------------------------------------------------------------
def border_strip(gh, gw, n_unknown, side="top"):
    """A free strip 3 cells thick along one border of an occupied map, one row (column) in, with n_unknown unknown cells
    between it and the border.  The frontier is those cells; its dilation is clipped by the border to (n_unknown + 2) x 2."""
    if side in ("left", "right"):
        lab = border_strip(gw, gh, n_unknown, "top" if side == "left" else "bottom")
        return np.ascontiguousarray(lab.T)
    lab = np.full((gh, gw), OCCUPIED, dtype=np.uint8)
    c = gw // 2 - 15
    lab[1:4, c:c + 30] = FREE
    lab[0, c + 9:c + 9 + n_unknown] = UNKNOWN
    return np.ascontiguousarray(lab[::-1]) if side == "bottom" else lab


# ---- a component whose smallest index is far from its bulk --------------------------------------------------------------
def comb(gh, gw):
    """Teeth pointing up from a slab along the bottom; one 3-cell-wide tooth on the right reaches row 1, so the component's
    smallest linear index lies far (many workgroups) from most of its cells.  A smaller free rectangle sits before it in
    raster order.  Background unknown."""
    lab = np.full((gh, gw), UNKNOWN, dtype=np.uint8)
    lab[gh - 12:gh - 2, 3:gw - 3] = FREE
    for k, c in enumerate(range(6, gw - 20, 9)):
        lab[gh - 12 - 8 - 5 * (k % 3):gh - 12, c:c + 4] = FREE
    lab[1:gh - 12, gw - 9:gw - 6] = FREE                                # the tall tooth
    lab[1:9, 5:25] = FREE                                               # decoy: first in raster order, 160 cells
    return lab


# ---- independent checkers (no scipy.ndimage.label) ------------------------------------------------------------------------
def _shifted(a, dy, dx, fill):
    out = np.full_like(a, fill)
    h, w = a.shape
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    out[yd, xd] = a[ys, xs]
    return out


def erode3(a):
    """3 x 3 erosion, cells outside the image do not constrain."""
    a = np.asarray(a, dtype=bool)
    out = np.ones_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out &= _shifted(a, dy, dx, True)
    return out


def dilate3(a):
    a = np.asarray(a, dtype=bool)
    out = np.zeros_like(a)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out |= _shifted(a, dy, dx, False)
    return out


def open3(a):
    return dilate3(erode3(a))


def flood_components(mask, diagonals="both"):
    """Labels (1.. in raster order of each component's first cell, 0 background) and sizes, by an iterative flood fill.
    diagonals: "both" (8-connected), "none" (4-connected), "main" (only up-left / down-right), "anti" (only up-right / down-left)."""
    mask = np.asarray(mask, dtype=bool)
    h, w = mask.shape
    lab = np.zeros((h, w), dtype=np.int32)
    nb = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if diagonals in ("both", "main"):
        nb += [(-1, -1), (1, 1)]
    if diagonals in ("both", "anti"):
        nb += [(-1, 1), (1, -1)]
    sizes = []
    for y0, x0 in zip(*np.where(mask)):
        if lab[y0, x0]:
            continue
        cur = len(sizes) + 1
        lab[y0, x0] = cur
        stack, n = [(int(y0), int(x0))], 0
        while stack:
            y, x = stack.pop()
            n += 1
            for dy, dx in nb:
                yy, xx = y + dy, x + dx
                if 0 <= yy < h and 0 <= xx < w and mask[yy, xx] and not lab[yy, xx]:
                    lab[yy, xx] = cur
                    stack.append((yy, xx))
        sizes.append(n)
    return lab, np.asarray(sizes, dtype=np.int64)


def expected_free_space(label):
    """build_connected_freespace without points, on the checkers above: opening, largest component, ties to the first."""
    lab, sizes = flood_components(open3(np.asarray(label) == FREE))
    if len(sizes) == 0:
        return np.zeros(lab.shape, dtype=np.uint8)
    return (lab == 1 + int(np.argmax(sizes))).astype(np.uint8)


def frontier_components(label, free_space, min_area=10):
    """(frontier mask, labels of its dilation, sizes of all components, qualifying labels) as build_frontiers defines them."""
    free_space = np.asarray(free_space, dtype=bool)
    frontier = dilate3(free_space) & ~free_space & (np.asarray(label) == UNKNOWN)
    lab, sizes = flood_components(dilate3(frontier))
    return frontier, lab, sizes, 1 + np.where(sizes > min_area)[0]


def selection_keys(lab, sizes, qualifying, cam_pos, method):
    """The key build_frontiers maximises per qualifying component, in label order: `combined` size / (mean distance + 20),
    `closest` minus the mean distance, `largest` the size."""
    keys = []
    for l in qualifying:
        pos = np.stack(np.where(lab == l), axis=1).astype(np.float64)
        mean = np.linalg.norm(pos - np.asarray(cam_pos, dtype=np.float64)[None], axis=1).mean()
        c = float(sizes[l - 1])
        keys.append(c if method == "largest" else c / (mean + 20.0) if method == "combined" else -mean)
    return np.asarray(keys, dtype=np.float64)


def key_gap(keys):
    """Relative gap between the best and the second-best key (inf with fewer than two)."""
    if len(keys) < 2:
        return np.inf
    s = np.sort(keys)[::-1]
    return float((s[0] - s[1]) / abs(s[0]))


# ---- the catalogue both test files walk: name -> (label image, camera cell (row, col)) ----------------------------------
_CASES = None


def cases():
    """Built once and shared; the arrays are read-only."""
    global _CASES
    if _CASES is None:
        c = {
            "serpentine": (serpentine(193, 257), (101, 77)),
            "serpentine_t": (serpentine_t(193, 257), (60, 140)),
            "spiral": (spiral(193, 257), (88, 131)),
            "diagonal": (diagonal_chains(193, 257), (150, 90)),
            "diagonal_mirror": (diagonal_chains(193, 257, mirror=True), (150, 90)),
            "rectangles2": (equal_rectangles(97, 130, 2), (50, 61)),
            "rectangles3": (equal_rectangles(97, 130, 3), (50, 61)),
            "gapped_room": (gapped_room(97, 130), (43, 71)),
            "perforated": (perforated_slab(97, 130), (51, 58)),
            "perforated_full": (perforated_slab(97, 130, full=True), (51, 58)),
            "comb": (comb(193, 257), (120, 100)),
        }
        for side in ("top", "bottom", "left", "right"):
            for n in (3, 4):
                c[f"strip_{side}_{n}"] = (border_strip(97, 130, n, side), (47, 59))
        for lab, _ in c.values():
            lab.setflags(write=False)
        _CASES = c
    return _CASES
