"""Cases for DBSCAN and the target selection of global_planning (csrc/fr_cluster_math.h, csrc/fr_cluster.hip), shared by
tests/test_cluster_cpu.py, tests/test_gpu_cluster.py and tests/golden/make_dbscan_vectors.py.

  * `make_case(family, N, seed)` -- seeded clouds; `qualifying_case` draws seeds until `qualifies()` holds;
  * `restate_dbscan` -- the labelling rule of fr_cluster_math.h in NumPy / cKDTree with float64 distances on the float32 inputs;
  * `restate_select` -- gaussian.py:1221-1267 as a torch + restatement chain;
  * the g++ harness over the header (tests/harness/fr_cluster_harness.cpp) and its wrappers.

`qualifies()`: no pair distance lies within relative 2e-6 of eps.  The binary32 expression d2 = (dx dx + dy dy) + dz dz against
the float64 distance of the same float32 inputs is off by at most 8 roundings of 2^-24 = 4.8e-7 relative (three subtractions, three
squares, two sums); the margin is four times that.  Under it binary32 and float64 decide every pair alike, so the labels must be
EQUAL.  For selection cases additionally no band score lies within 4 ulp of the threshold, unless the rank is integral (then the
threshold IS a score and the strict comparison is exact)."""
import ctypes
import os

import numpy as np
import harness_build

F = np.float32
EPS, MIN_SAMPLES = 0.1, 5
REL_MARGIN = 2e-6
MAX_SEEDS = 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# family -> sizes: wave edges (63 / 64 / 65), workgroup edges (257, 1025), about 5000
FAMILIES = {
    "blobs": (63, 64, 65, 257, 1025, 5000),
    "chain": (2000,),
    "bridge": (17,),
    "straddle": (600,),
    "dense": (4096,),
    "outlier": (1025,),
    "nonfinite": (1025,),
    "permuted": (1025,),
    "tiny": (0, 1, 4, 5),
}
# (family, N, eps, min_samples): what tests/golden/dbscan_cases.npz holds sklearn's labels for
FAMILY_MIN_SAMPLES = {"chain": 3, "straddle": 2}        # a chain point has two neighbours and itself; a straddling pair only each other
GOLDEN = [(f, n, EPS, FAMILY_MIN_SAMPLES.get(f, MIN_SAMPLES)) for f, sizes in FAMILIES.items() for n in sizes if n > 0] + \
         [("blobs", 1025, EPS, 1), ("blobs", 1025, EPS, 2), ("blobs", 1025, EPS, 8), ("blobs", 257, 0.05, 3), ("blobs", 65, EPS, 100)]


def _blobs(rng, n, spread=0.05, box=1.5, noise=0.25):
    k = max(1, n // 120)
    centres = rng.uniform(-box, box, (k, 3))
    n_noise = int(noise * n)
    pts = centres[rng.integers(0, k, n - n_noise)] + rng.normal(size=(n - n_noise, 3)) * spread * np.array([1.0, 0.3, 2.0])
    pts = np.concatenate([pts, rng.uniform(-box - 0.5, box + 0.5, (n_noise, 3))])
    return pts[rng.permutation(n)]


def make_case(family, N, seed=0):
    """float32 [N,3]"""
    rng = np.random.default_rng([sum(map(ord, family)), N, seed])
    if family in ("blobs", "permuted"):
        pts = _blobs(rng, N)
    elif family == "chain":
        # one point every 0.09 along a slanted line: about 180 m, so it crosses every kind of cell edge and many workgroups
        t = np.arange(N)[:, None] * 0.09
        d = np.array([0.62, -0.35, 0.70])
        pts = -40.0 + t * d / np.linalg.norm(d) + rng.normal(size=(N, 3)) * 1e-4
        pts = pts[rng.permutation(N)]
    elif family == "bridge":
        # two rows of eight core points (0.02 apart) whose ends are 0.19 apart, and one point between them that is within eps of
        # the end of each and of nothing else: three neighbours, not core.  The second row comes first, so it is cluster 0.
        a = np.zeros((8, 3))
        a[:, 0] = -0.02 * np.arange(8)
        b = np.zeros((8, 3))
        b[:, 0] = 0.19 + 0.02 * np.arange(8)
        mid = np.array([[0.095, 0.0, 0.0]])
        pts = np.concatenate([b, mid, a]) + rng.normal(size=(17, 3)) * 1e-5 - 0.3
    elif family == "straddle":
        # pairs about eps apart placed across the edges of the cells of side 1.125 eps, in the negative octant
        side = 1.125 * EPS
        edge = -3.0 + side * rng.integers(1, 20, (N // 2, 3))
        off = rng.uniform(0.2, 0.98, (N // 2, 1)) * EPS * _unit(rng, N // 2)
        p = edge - off * rng.uniform(0.0, 1.0, (N // 2, 1))
        pts = np.concatenate([p, p + off])
        pts = np.concatenate([pts, pts[:N - len(pts)]]) if len(pts) < N else pts[:N]
    elif family == "dense":
        pts = 0.7 + _unit(rng, N) * (EPS / 2) * rng.uniform(0, 1, (N, 1)) ** (1 / 3)
    elif family == "outlier":
        pts = _blobs(rng, N)
        pts[N // 2] = [1e6, -2e5, 3.0]
    elif family == "nonfinite":
        pts = _blobs(rng, N)
        bad = rng.choice(N, 40, replace=False)
        pts[bad[:15], rng.integers(0, 3, 15)] = np.nan
        pts[bad[15:30], rng.integers(0, 3, 15)] = np.inf
        pts[bad[30:], rng.integers(0, 3, 10)] = -np.inf
    elif family == "tiny":
        pts = np.tile(rng.uniform(-1, 1, (1, 3)), (N, 1)) if N == 5 else rng.uniform(-1, 1, (N, 3)) * 0.03     # 5: identical points
    else:
        raise ValueError(family)
    return np.ascontiguousarray(pts, F).reshape(N, 3)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _finite(pts):
    return np.isfinite(pts).all(1)


def qualifies(pts, eps=EPS, margin=REL_MARGIN):
    """no pair of finite points at a float64 distance within relative `margin` of eps"""
    from scipy.spatial import cKDTree
    p = pts[_finite(pts)].astype(np.float64)
    if len(p) < 2:
        return True
    if np.abs(p).max() > 1e5:                                 # the tree's own arithmetic: keep far outliers out of it
        p = p[np.abs(p).max(1) <= 1e5]
    tree = cKDTree(p)
    e = float(F(eps))
    outer = tree.count_neighbors(tree, e * (1 + margin))
    inner = tree.count_neighbors(tree, e * (1 - margin))
    return outer == inner


def qualifying_case(family, N, eps=EPS):
    for seed in range(MAX_SEEDS):
        pts = make_case(family, N, seed)
        if qualifies(pts, eps):
            return pts, seed
    raise AssertionError(f"no qualifying {family} case of {N} points in {MAX_SEEDS} seeds")


def restate_dbscan(pts, eps=EPS, min_samples=MIN_SAMPLES):
    """the labelling rule of csrc/fr_cluster_math.h with float64 distances on the float32 inputs: int32 [N]"""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    N = len(pts)
    labels = np.full(N, -1, np.int32)
    ok = np.nonzero(_finite(pts))[0]
    if len(ok) == 0:
        return labels
    p = pts[ok].astype(np.float64)
    e = float(F(eps))
    tree = cKDTree(p)
    counts = tree.query_ball_point(p, e, return_length=True)                 # itself included, <=
    core = counts >= min_samples
    pairs = tree.query_pairs(e, output_type="ndarray")
    n = len(ok)
    cc = pairs[core[pairs[:, 0]] & core[pairs[:, 1]]] if len(pairs) else np.zeros((0, 2), np.int64)
    _, comp = connected_components(coo_matrix((np.ones(len(cc)), (cc[:, 0], cc[:, 1])), shape=(n, n)), directed=False)
    lab = np.full(n, -1, np.int64)
    core_idx = np.nonzero(core)[0]
    if len(core_idx):
        # number the components by the lowest (original = ascending here) index of their core points
        first = {}
        for i in core_idx:
            first.setdefault(comp[i], len(first))
        lab[core_idx] = [first[comp[i]] for i in core_idx]
        big = np.iinfo(np.int64).max
        best = np.full(n, big)
        for a, b in ((pairs[:, 0], pairs[:, 1]), (pairs[:, 1], pairs[:, 0])) if len(pairs) else ():
            m = core[b] & ~core[a]
            np.minimum.at(best, a[m], lab[b[m]])
        border = (~core) & (best != big)
        lab[border] = best[border]
    labels[ok] = lab
    return labels


def same_partition(a, b):
    """two labellings describe the same clusters (numbering aside) and the same noise"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a < 0, b < 0):
        return False
    m = a >= 0
    pairs = set(zip(a[m].tolist(), b[m].tolist()))
    return len(pairs) == len(set(p[0] for p in pairs)) == len(set(p[1] for p in pairs))


# ---- selection ------------------------------------------------------------------------------------------------------------------------

SELECT_P = 20000
LOWER_Y, UPPER_Y, Q = -0.3, 0.3, 0.8


def make_select_case(P=SELECT_P, seed=0, kind="map"):
    """(means3D [P,3], scores [P]) float32: the means of a fisher_rast.synthetic room with a few dense clumps of high score inside
    the band (the room alone is too sparse at this size for a cluster at eps = 0.1); kind "equal": every score the same"""
    import sys
    pkg = os.path.join(ROOT, "fisher-nerf-customized_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    from fisher_rast import synthetic
    rng = np.random.default_rng([P, seed, 91])
    means = synthetic.room_shell(P, seed=seed + 3)["means3D"].numpy().copy()
    scores = rng.uniform(0.05, 1.0, P)
    n_clump = P // 8
    rows = rng.choice(P, n_clump, replace=False)
    centres = np.stack([rng.uniform(-4, 4, 6), rng.uniform(-0.2, 0.2, 6), rng.uniform(-4, 4, 6)], 1)
    which = rng.integers(0, 6, n_clump)
    means[rows] = centres[which] + rng.normal(size=(n_clump, 3)) * 0.06
    scores[rows] = rng.uniform(0.9, 2.0, n_clump) + 0.3 * which
    if kind == "equal":
        scores[:] = 0.75
    return np.ascontiguousarray(means, F), np.ascontiguousarray(scores, F)


def restate_select(means, scores, lower_y=LOWER_Y, upper_y=UPPER_Y, q=Q, eps=EPS, min_samples=MIN_SAMPLES):
    """gaussian.py:1221-1267 with torch on the CPU and the restatement in DBSCAN's place; dict of arrays and status values"""
    import torch
    m, s = torch.from_numpy(means), torch.from_numpy(scores)
    sign = torch.bitwise_and(m[:, 1] >= lower_y, m[:, 1] <= upper_y)
    band_idx = torch.where(sign)[0]
    sel_scores = s[sign]
    threshold = torch.quantile(sel_scores, q)
    above = sel_scores > threshold
    above_idx = band_idx[above]
    out = dict(band_idx=band_idx.numpy().astype(np.int32), above_idx=above_idx.numpy().astype(np.int32), threshold=threshold.numpy().astype(F),
               argmax=int(band_idx[torch.argmax(sel_scores)]), labels=np.zeros(0, np.int32), max_label=-1, n_clusters=0,
               selected_idx=np.zeros(0, np.int32))
    if len(above_idx):
        labels = restate_dbscan(means[above_idx.numpy()], eps, min_samples)
        sc = sel_scores[above].numpy()
        max_label, max_score = -1, -1
        for lab in np.unique(labels):
            if lab < 0:
                continue
            cs = sc[labels == lab].max()
            if cs > max_score:
                max_label, max_score = int(lab), cs
        out.update(labels=labels, max_label=max_label, n_clusters=int(labels.max()) + 1, selected_idx=out["above_idx"][labels == max_label])
    return out


def qualifies_select(means, scores, lower_y=LOWER_Y, upper_y=UPPER_Y, q=Q, eps=EPS):
    import torch
    band = (means[:, 1] >= lower_y) & (means[:, 1] <= upper_y)
    s = scores[band]
    if len(s) == 0 or np.isnan(s).any():
        return False
    thr = torch.quantile(torch.from_numpy(s), q).numpy().astype(F)
    rank = F(q) * F(len(s) - 1)
    if rank != np.floor(rank):
        ulp = np.spacing(np.abs(thr))
        if (np.abs(s.astype(np.float64) - float(thr)) <= 4 * float(ulp)).any():
            return False
    return qualifies(means[band][s > thr], eps)


def qualifying_select_case(P=SELECT_P, kind="map"):
    for seed in range(MAX_SEEDS):
        means, scores = make_select_case(P, seed, kind)
        if kind == "equal" or qualifies_select(means, scores):
            return means, scores, seed
    raise AssertionError("no qualifying selection case")


# ---- the g++ harness --------------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_cluster_harness"))
    vp, f32, i32, u32 = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_uint32
    h.frk_h_eps_ok.argtypes, h.frk_h_eps_ok.restype = [f32], i32
    h.frk_h_dist2.argtypes, h.frk_h_dist2.restype = [vp, vp], f32
    h.frk_h_inside.argtypes, h.frk_h_inside.restype = [vp, vp, f32], i32
    h.frk_h_side.argtypes, h.frk_h_side.restype = [f32, f32, f32], f32
    h.frk_h_cell.argtypes, h.frk_h_cell.restype = [f32, f32, f32], u32
    h.frk_h_cells.argtypes, h.frk_h_cells.restype = [i32, vp, f32, vp, vp], None
    h.frk_h_dbscan.argtypes, h.frk_h_dbscan.restype = [i32, vp, f32, i32, vp, vp], None
    h.frk_h_quantile_rank.argtypes, h.frk_h_quantile_rank.restype = [f32, u32, vp, vp], None
    h.frk_h_lerp.argtypes, h.frk_h_lerp.restype = [f32, f32, f32], f32
    h.frk_h_quantile.argtypes, h.frk_h_quantile.restype = [u32, vp, f32], f32
    h.frk_h_winner.argtypes, h.frk_h_winner.restype = [i32, vp, vp], i32
    h.frk_h_target_select.argtypes, h.frk_h_target_select.restype = [i32, vp, vp, f32, f32, f32, f32, i32] + [vp] * 6, None
    return h


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def harness_dbscan(h, pts, eps=EPS, min_samples=MIN_SAMPLES):
    """(labels int32 [N], status int32 [8]) of the brute-force DBSCAN over the header"""
    pts = np.ascontiguousarray(pts, F)
    labels, status = np.zeros(max(len(pts), 1), np.int32), np.zeros(8, np.int32)
    h.frk_h_dbscan(len(pts), _p(pts), eps, min_samples, _p(labels), _p(status))
    return labels[:len(pts)], status


def harness_cells(h, pts, eps=EPS):
    pts = np.ascontiguousarray(pts, F)
    cells, sides = np.zeros((max(len(pts), 1), 3), np.uint32), np.zeros(3, F)
    h.frk_h_cells(len(pts), _p(pts), eps, _p(cells), _p(sides))
    return cells[:len(pts)], sides


def harness_quantile(h, x, q=Q):
    x = np.ascontiguousarray(x, F)
    return F(h.frk_h_quantile(len(x), _p(x), q))


def harness_winner(h, scores, labels):
    scores, labels = np.ascontiguousarray(scores, F), np.ascontiguousarray(labels, np.int32)
    return int(h.frk_h_winner(len(scores), _p(scores), _p(labels)))


STATUS_NAMES = ("n_band", "n_above", "n_clusters", "max_label", "n_selected", "argmax")


def decode_status(words):
    """the 16 int32 words of fr_target_select as a dict"""
    w = np.ascontiguousarray(words, np.int32).reshape(-1)
    d = {k: int(w[i]) for i, k in enumerate(STATUS_NAMES)}
    d.update(sides=w[6:9].copy().view(F), nan=int(w[9]), threshold=w[10:11].copy().view(F)[0], n_finite=int(w[11]))
    return d


def harness_select(h, means, scores, lower_y=LOWER_Y, upper_y=UPPER_Y, q=Q, eps=EPS, min_samples=MIN_SAMPLES):
    means, scores = np.ascontiguousarray(means, F), np.ascontiguousarray(scores, F)
    P = len(means)
    lists = [np.zeros(max(P, 1), np.int32) for _ in range(4)]
    thr, status = np.zeros(1, F), np.zeros(16, np.int32)
    h.frk_h_target_select(P, _p(means), _p(scores), lower_y, upper_y, q, eps, min_samples, *[_p(a) for a in lists], _p(thr), _p(status))
    s = decode_status(status)
    return dict(band_idx=lists[0][:s["n_band"]], above_idx=lists[1][:s["n_above"]], labels=lists[2][:s["n_above"]],
                selected_idx=lists[3][:s["n_selected"]], threshold=thr[0], status=s, words=status)
