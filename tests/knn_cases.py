"""Cases of simple-knn (fr_knn_dist2) and of the Z-curve order (fr_spatial_order): seeded generators, the NumPy restatement of
k_knn_morton, key patterns for the sorting network, and the qualification checks (conditions on a case, not on the code).

The statement of fr_knn_dist2 is the project's brute-force oracle (oracle/fisher_oracle.c, orc_knn_dist2): the same binary32
arithmetic in the same order, so every comparison is bit for bit.  The statement of fr_spatial_order is
np.argsort(morton_np(points), kind="stable").

Sizes: 64 = a wave and a sub-box, 1024 = a box, 2048 = an LDS chunk of the sorting network, 4096 / 8192 / 65536 = powers of two
of the network's global stages, 6145 = three chunks and one key (neither a power of two nor one past one), 65536 = what the 256
workgroups of the bounding-box reduction cover without striding."""
import numpy as np

F = np.float32
FAMILIES = ("uniform", "clusters", "lattice", "plane", "line", "point", "stretch", "seam", "dup_groups", "nonfinite", "offset", "overflow")
KNN_SWEEP = (2, 4, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8192, 8193, 16385)
KNN_PAST_THE_GRID_CAP = 65537
ORDER_SWEEP = (63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 6145, 8192, 8193, 65536, 65537, 131073)
SEAM_SIZES = (4097, 8193, 16385)
LATTICE_SIDES = (13, 17)                                  # 2197 and 4913 points
LATTICE_ANSWER = F(0.0625)                                # three neighbours at 0.25, corners included: (3 * 0.0625) / 3, exact
KNN_FAMILY_SIZES = dict(lattice=tuple(s ** 3 for s in LATTICE_SIDES), plane=(1025, 5000), line=(1025, 5000), point=(4, 65, 2049),
                        stretch=(2049, 5000), seam=SEAM_SIZES, dup_groups=(257, 5000), nonfinite=(1025, 5000), offset=(1025, 5000),
                        overflow=(1025, 5000))
ORDER_FAMILY_SIZES = dict(plane=(1025, 5000), line=(1025, 5000), point=(65, 2049), stretch=(2049, 5000), nonfinite=(1025, 5000))
PATTERN_SIZES = (2049, 4097, 8193)
PATTERNS = ("equal", "descending", "ones-then-zeros", "alternating", "one-in-front", "zero-at-the-end", "random-1/2", "random-1/64")
METAMORPHIC_P = 4097
METAMORPHIC_SEED = 3                                      # the first seed at which the oracle itself obeys the scaling law (scaling_mismatches)
SCALING_P = 3000

# the qualification bounds
SEAM_FAR_BOX, SEAM_FAR_SUB = 0.30, 0.80                   # a neighbour >= 1024 ranks away / >= 64 ranks away
STRETCH_CODE0 = 0.999


def _rng(family, P, seed):
    return np.random.default_rng([FAMILIES.index(family), P, seed])


def dup_group_rows(P, seed=0):
    """the rows of `dup_groups` that are made identical: a list of index arrays, sizes 2, 3, 4, 5 in turn, disjoint"""
    rng = np.random.default_rng([FAMILIES.index("dup_groups"), P, seed, 1])
    n_groups = max(4, min(16, P // 64) // 4 * 4)
    sizes = [2 + g % 4 for g in range(n_groups)]
    rows = rng.permutation(P)[:sum(sizes)]
    return [np.sort(r) for r in np.split(rows, np.cumsum(sizes)[:-1])]


def nonfinite_rows(P, seed=0):
    """(rows, axes, kind indices into (NaN, +inf, -inf)) of `nonfinite`: about 5 % of the rows, one coordinate each"""
    rng = np.random.default_rng([FAMILIES.index("nonfinite"), P, seed, 1])
    rows = np.flatnonzero(rng.uniform(size=P) < 0.05)
    if rows.size < 3:
        rows = np.arange(min(3, P))
    kinds = np.arange(rows.size) % 3                      # every kind occurs
    return rows, rng.integers(0, 3, rows.size), kinds


def make_cloud(family, P, seed=0, kinds=(np.nan, np.inf, -np.inf)):
    """float32 [P, 3], seeded by (family, P, seed).  `kinds`: the values `nonfinite` draws from, in turn."""
    rng = _rng(family, P, seed)
    if family == "uniform":
        m = rng.uniform(-2, 2, (P, 3))
    elif family == "clusters":
        m = rng.normal(size=(P, 3))
        m[:P // 4] *= 0.01                                # a dense region
        n_dup = min(50, P // 8)
        m[P // 2:P // 2 + n_dup] = m[0]                   # exact copies: zero distances
    elif family == "lattice":
        s = int(round(P ** (1 / 3)))
        assert s ** 3 == P and s >= 2, "lattice: P is a cube"
        g = np.stack(np.meshgrid(*(np.arange(s),) * 3, indexing="ij"), -1).reshape(-1, 3) * 0.25
        m = g[rng.permutation(P)]
    elif family in ("plane", "line", "point"):
        m = rng.uniform(-2, 2, (P, 3))
        held = rng.permutation(3)[:dict(plane=1, line=2, point=3)[family]]
        m[:, held] = rng.uniform(-2, 2, 3)[held]
    elif family == "stretch":
        m = rng.uniform(0, 1, (P, 3))
        m[rng.integers(0, P)] = 1e6
    elif family == "seam":
        m = rng.uniform(-1, 1, (P, 3))
        i = np.arange(P)
        m[i, i % 3] = rng.uniform(-0.004, 0.004, P)
        m[0], m[1] = -1.0, 1.0                            # the corners pin the frame: the seams are the planes through 0
    elif family == "dup_groups":
        m = rng.normal(size=(P, 3))
        for rows in dup_group_rows(P, seed):
            m[rows] = m[rows[0]]
    elif family == "nonfinite":
        m = rng.normal(size=(P, 3))
    elif family == "offset":
        m = rng.normal(size=(P, 3)) * 0.01 + np.array([1000.0, -500.0, 2000.0])
    elif family == "overflow":
        m = rng.normal(size=(P, 3)).astype(F).astype(np.float64) * 2.0 ** 70
    else:
        raise KeyError(family)
    m = m.astype(F)
    if family == "nonfinite":
        rows, axes, k = nonfinite_rows(P, seed)
        m[rows, axes] = np.asarray(kinds, F)[k % len(kinds)]
    return m


# ---- the Z-curve ----------------------------------------------------------------------------------------------------------------------

def _spread(x):
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    x = (x | (x << 2)) & 0x09249249
    return x


def encode(q):
    """the 30-bit code of integer cells q [n, 3] (10 bits per axis, x lowest)"""
    q = np.asarray(q).astype(np.uint64)
    return _spread(q[:, 0]) | (_spread(q[:, 1]) << 1) | (_spread(q[:, 2]) << 2)


def morton_np(m):
    """k_knn_morton restated: 10 bits per axis over the bounding box, x lowest.  The bounds are taken with fmin / fmax, which ignore
    NaN (k_knn_minmax); an axis of zero, infinite-negative or NaN extent gives 0; a NaN quotient (a NaN coordinate, inf / inf,
    inf - inf) quantises to 0 (fminf(fmaxf(u, 0), 1) returns the number of a (NaN, number) pair)."""
    m = np.asarray(m).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        lo, hi = np.fmin.reduce(m, 0), np.fmax.reduce(m, 0)
        ext = (hi - lo).astype(F)
        ok = ext > 0
        u = np.where(ok, (m - lo) / np.where(ok, ext, 1), 0).astype(F)
        u = np.where(np.isnan(u), F(0), u)
        q = (np.clip(u, 0, 1) * F(1023.0)).astype(np.uint32)
    return encode(q)


def z_order(m):
    """what fr_spatial_order returns: a stable sort by code"""
    return np.argsort(morton_np(m), kind="stable")


def z_rank(m):
    order = z_order(m)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return rank


# ---- key patterns for the sorting network -----------------------------------------------------------------------------------------------
# The network is data-oblivious, so a wrong comparator shows on 0-1 inputs.  Row 0 and row P - 1 are the corners of the frame (in either order), cells
# (0, 0, 0) and (1023, 1023, 1023); every other row sits at the centre of a cell 0 .. 1022 per axis, so its code is the wanted one.

ZERO_CELL, ONE_CELL = (5, 0, 0), (7, 3, 1022)
EQUAL_CELL = (500, 0, 0)


def pattern_codes(pattern, P, seed=0):
    """(cells int64 [P, 3], codes uint64 [P]) of a pattern"""
    rng = np.random.default_rng([PATTERNS.index(pattern), P, seed, 2])
    n = P - 2
    lo, hi = np.zeros((1, 3), np.int64), np.full((1, 3), 1023, np.int64)
    if pattern == "descending":
        cells = rng.integers(0, 1023, (4 * n, 3))
        _, first = np.unique(encode(cells), return_index=True)
        cells = cells[first[:n]][::-1]                    # np.unique sorts: strictly ascending codes, reversed
        assert len(cells) == n
        q = np.concatenate([hi, cells, lo])               # the whole array descends
    else:
        if pattern == "equal":
            one = np.zeros(n, bool)
        elif pattern == "ones-then-zeros":
            one = np.arange(n) < n // 2
        elif pattern == "alternating":
            one = np.arange(n) % 2 == 0
        elif pattern == "one-in-front":
            one = np.arange(n) == 0
        elif pattern == "zero-at-the-end":
            one = np.arange(n) != n - 1
        elif pattern == "random-1/2":
            one = rng.uniform(size=n) < 0.5
        elif pattern == "random-1/64":
            one = rng.uniform(size=n) < 1 / 64
        else:
            raise KeyError(pattern)
        mid = np.where(one[:, None], np.array(ONE_CELL), np.array(EQUAL_CELL if pattern == "equal" else ZERO_CELL))
        # "equal" is already sorted; the two-valued patterns have the corners swapped, so that the last key -- the one past a chunk
        # and past a power of two -- has to travel to the front
        q = np.concatenate([lo, mid, hi] if pattern == "equal" else [hi, mid, lo])
    return q, encode(q)


def pattern_points(pattern, P, seed=0):
    """float32 [P, 3] whose codes are pattern_codes(pattern, P, seed)[1]"""
    q, _ = pattern_codes(pattern, P, seed)
    m = q.astype(F) + F(0.5)
    corner = (q == 0).all(1) | (q == 1023).all(1)
    m[corner] = q[corner]
    return m


# ---- qualification ----------------------------------------------------------------------------------------------------------------------

def far_neighbour_fractions(m):
    """fractions of the points with one of their three nearest neighbours (float64, SciPy) at least 1024 / at least 64 ranks away"""
    from scipy.spatial import cKDTree
    m64 = np.asarray(m, np.float64)
    _, nn = cKDTree(m64).query(m64, k=4)
    rank = z_rank(m)
    gap = np.abs(rank[nn[:, 1:]] - rank[:, None]).max(1)
    return float((gap >= 1024).mean()), float((gap >= 64).mean())


def code0_fraction(m):
    return float((morton_np(m) == 0).mean())


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def scaled(a, e):
    """a * 2^e in binary32 (exact for the clouds here: no coordinate leaves the normal range)"""
    return (np.asarray(a, F) * F(2.0 ** e)).astype(F)


def scaling_mismatches(knn, m, e=50):
    """rows at which knn(m * 2^+-e) is not knn(m) * 2^+-2e bit for bit, for both signs.  The law holds for every operation whose
    result stays normal; a squared coordinate difference that goes subnormal under 2^-e rounds on its own and may move the sum's
    last bit (the `clusters` cloud of seed 0 has two such rows in the oracle itself), so a cloud is qualified with the oracle."""
    base = knn(m)
    return [int((bits(knn(scaled(m, s))) != bits(scaled(base, 2 * s))).sum()) for s in (e, -e)]


def metamorphic_cloud():
    return make_cloud("clusters", METAMORPHIC_P, METAMORPHIC_SEED)
