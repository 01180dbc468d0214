"""Cases of the POp-GS block stage (fr_raster_cfg.ext of fr_fisher_views; csrc/fr_popgs_block.hip, fr_popgs_block_math.h), shared by
tests/test_popgs_block_cpu.py (the g++ harness) and tests/test_gpu_popgs_block.py (the kernels): synthetic probe rows, priors and
masks; the binary64 NumPy restatement (np.linalg.inv / slogdet on the promoted float32 inputs); the bound.

The bound (u = 2^-53, kappa = np.linalg.cond of the binary64 block).  An unpivoted L D L^T of a d x d block commits a backward error of
about (d + 1) u |A|; to first order trace(A^-1) then moves by kappa (d + 1) u |trace(A^-1)| and log det by d (d + 1) u kappa.  The
kernel and LAPACK each commit one such error; the factor 8 covers both with a margin of about 2:
    T-opt, per pose:  sum_b 8 (d + 1) u kappa(A1) |t_b|
    D-opt, per pose:  sum_b 8 d (d + 1) u (kappa(A1) + kappa(A0))
plus 2^-50 sum |terms| for the order of the sums.  The cases keep kappa <= 1e9 (asserted in `restate`)."""
import ctypes
import itertools

import numpy as np

import harness_build

U = 2.0 ** -53
KAPPA_MAX = 1e9
ROW_BLOCKS = {"mean": (0, 3), "opacity": (3, 4), "rot": (7, 11), "scale": (4, 7)}          # gaussian_object._ROW_BLOCKS
BLOCK_ORDER = ("mean", "opacity", "rot", "scale")                                            # gaussian_object._POPGS_BLOCK_ORDER
FLAG_SETS = [dict(use_opacity=bool(o), use_rot=bool(r), use_scale=bool(s)) for o, r, s in itertools.product((0, 1), repeat=3)]
TOPT, DOPT = 0, 1


def flag_id(f):
    return "".join(k[4] for k, v in f.items() if v) or "mean"


def columns(use_opacity=True, use_rot=True, use_scale=True):
    want = {"mean": True, "opacity": use_opacity, "rot": use_rot, "scale": use_scale}
    return [c for n in BLOCK_ORDER if want[n] for c in range(*ROW_BLOCKS[n])]


def sym_lower(B):
    """the symmetric matrix whose lower triangle is B's (stacked [.., d, d])"""
    L = np.tril(B)
    return L + np.swapaxes(np.tril(B, -1), -1, -2)


def np_pivots(A):
    """pivots of the unpivoted L D L^T of one symmetric binary64 matrix"""
    A = np.array(A, dtype=np.float64)
    d = A.shape[0]
    piv = np.zeros(d)
    for j in range(d):
        piv[j] = A[j, j]
        l = A[j + 1:, j] / piv[j]
        A[j + 1:, j + 1:] -= np.outer(l, A[j + 1:, j])
    return piv


def rn32(x):
    """a Fraction rounded to the nearest binary32 (ties to even; normal range), exactly"""
    from fractions import Fraction
    if x == 0:
        return np.float32(0.0)
    e = 0
    a = abs(x)
    while a >= 1 << 24:
        a, e = a / 2, e + 1
    while a < 1 << 23:
        a, e = a * 2, e - 1
    n = a.numerator // a.denominator
    rem = a - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    v = Fraction(n) * (Fraction(2) ** e)
    return np.float32(float(v if x > 0 else -v))                       # exact: at most 24 significant bits


def fma32(a, b, c):
    """fmaf(a, b, c) on binary32 values: the exact a b + c, rounded once"""
    from fractions import Fraction
    return rn32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def spd_blocks(rng, n, d, K):
    """float32 [n, d, d]: every third block a Gram matrix of rank <= K (what a keyframe gives: conditioned by lam alone), the others
    full rank; norms of a few units, so that with lam = 1e-6 kappa stays below ~1e8"""
    out = np.zeros((n, d, d), np.float32)
    for q in range(n):
        if q % 3 == 0:
            G = rng.uniform(-1.0, 1.0, (K, d)).astype(np.float32)
            out[q] = (G.T @ G / K).astype(np.float32)
        else:
            M = rng.uniform(-1.0, 1.0, (d, d))
            out[q] = (M @ M.T / d + 1e-3 * np.eye(d)).astype(np.float32)
    return out


def indefinite_block(rng, d):
    """float32 [d, d] = L D L^T, L unit lower with |l| <= 0.4, |D| in [0.5, 2] with both signs: the pivots stay well apart from 0"""
    L = np.tril(rng.uniform(-0.4, 0.4, (d, d)), -1) + np.eye(d)
    D = rng.uniform(0.5, 2.0, d) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
    return (L @ np.diag(D) @ L.T).astype(np.float32)


def make_case(seed, P, poses, K, n, flags, unsorted=True, vis_fraction=0.6):
    """dict(rows [poses K, P, 11] f32, prior [n, d, d] f32, idx [n] i32 (distinct, unsorted on request), vis [poses, P] u8, lam)"""
    rng = np.random.default_rng(seed)
    d = len(columns(**flags))
    rows = rng.uniform(-1.5, 1.5, (poses * K, P, 11)).astype(np.float32)
    rows *= rng.choice(np.array([1.0, 0.1, 3.0], np.float32), size=(1, P, 1))
    idx = rng.choice(P, size=n, replace=False).astype(np.int32)
    if not unsorted:
        idx.sort()
    vis = (rng.uniform(size=(poses, P)) < vis_fraction).astype(np.uint8)
    return dict(rows=rows, prior=spd_blocks(rng, n, d, K), idx=idx, vis=vis, lam=1e-6, P=P, poses=poses, K=K, n=n, flags=dict(flags), d=d)


def restate(case, criterion, kappa_max=KAPPA_MAX):
    """binary64 NumPy restatement of the SCORE mode: dict(scores [poses], matched [poses], bound [poses], skipped, kappa (largest))"""
    rows, prior, idx, vis, lam, K, P = (case[k] for k in ("rows", "prior", "idx", "vis", "lam", "K", "P"))
    cols = columns(**case["flags"])
    d = len(cols)
    poses = rows.shape[0] // K
    ok = (idx >= 0) & (idx < P)
    A0_all = sym_lower(prior.astype(np.float64)) + lam * np.eye(d)
    scores, matched, bound, worst = np.zeros(poses), np.zeros(poses, np.int64), np.zeros(poses), 0.0
    for p in range(poses):
        sel = np.nonzero(ok & (vis[p][np.clip(idx, 0, P - 1)] != 0))[0]
        matched[p] = sel.size
        if sel.size == 0:
            scores[p] = -np.inf
            continue
        G = rows[p * K:(p + 1) * K][:, idx[sel]][:, :, cols].astype(np.float64)              # [K, m, d]
        J = np.einsum("kvi,kvj->vij", G, G) / K
        A0 = A0_all[sel]
        A1 = A0 + J
        k0, k1 = np.linalg.cond(A0), np.linalg.cond(A1)
        worst = max(worst, float(k0.max()), float(k1.max()))
        if criterion == TOPT:
            terms = -np.trace(np.linalg.inv(A1), axis1=1, axis2=2)
            err = 8 * (d + 1) * U * k1 * np.abs(terms)
        else:
            terms = np.linalg.slogdet(A1)[1] - np.linalg.slogdet(A0)[1]
            err = 8 * d * (d + 1) * U * (k1 + k0)
        scores[p] = terms.sum()
        bound[p] = err.sum() + 2.0 ** -50 * np.abs(terms).sum()
    assert worst <= kappa_max, f"a case block has condition {worst:.3g}"
    return dict(scores=scores, matched=matched, bound=bound, skipped=int((~ok).sum()), kappa=worst)


def check_scores(got, want, what=""):
    """got [poses] against restate()'s result: -inf where no pair matched, else within the bound; returns the largest |error| / bound"""
    ratio = 0.0
    for p, (g, w, b) in enumerate(zip(np.asarray(got, np.float64), want["scores"], want["bound"])):
        if want["matched"][p] == 0:
            assert g == -np.inf, (what, p, g)
            continue
        assert np.isfinite(g), (what, p, g)
        r = abs(g - w) / b
        print(f"{what} pose {p}: got {g!r} want {w!r} |err| {abs(g - w):.3e} bound {b:.3e} ratio {r:.3f}")
        ratio = max(ratio, r)
    assert ratio <= 1.0, (what, ratio)
    return ratio


# ---- the g++ harness ----------------------------------------------------------------------------------------------------------------

def build_harness():
    h = ctypes.CDLL(harness_build.shared("fr_popgs_block_harness"))
    i, ll, dbl, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p
    h.frpbh_dim.restype, h.frpbh_dim.argtypes = i, [i, i, i]
    h.frpbh_cols.restype, h.frpbh_cols.argtypes = None, [i, i, i, vp]
    h.frpbh_factor.restype, h.frpbh_factor.argtypes = i, [i, vp, vp, vp, vp]
    h.frpbh_pair.restype, h.frpbh_pair.argtypes = i, [i, i, i, vp, ll, i, vp, dbl, i, vp]
    h.frpbh_prior_add.restype, h.frpbh_prior_add.argtypes = i, [i, i, i, vp, ll, i, i, vp]
    h.frpbh_scores.restype, h.frpbh_scores.argtypes = i, [i, i, i, i, i, i, i, vp, vp, vp, vp, dbl, i, vp, vp, vp]
    h.frpbh_ws_bytes.restype, h.frpbh_ws_bytes.argtypes = ctypes.c_ulonglong, [ll, ll]
    h.frpbh_constants.restype, h.frpbh_constants.argtypes = None, [vp]
    h.frpbh_layout.restype, h.frpbh_layout.argtypes = i, [vp]
    return h


def _orf(flags):
    return int(flags["use_opacity"]), int(flags["use_rot"]), int(flags["use_scale"])


def harness_factor(h, A):
    """(flag, pivots [d], trace(A^-1), sum log|pi|) of the header's factorisation of one symmetric binary64 matrix"""
    A = np.ascontiguousarray(A, np.float64)
    d = A.shape[0]
    piv, tr, la = np.zeros(d), ctypes.c_double(), ctypes.c_double()
    flag = h.frpbh_factor(d, A.ctypes.data, piv.ctypes.data, ctypes.addressof(tr), ctypes.addressof(la))
    assert flag >= 0
    return flag, piv, tr.value, la.value


def harness_scores(h, case, criterion):
    """(scores [poses] f64, matched [poses] i32, status [4] i32) of the SCORE mode through the header's arithmetic on the CPU"""
    rows, prior, idx, vis = (np.ascontiguousarray(case[k]) for k in ("rows", "prior", "idx", "vis"))
    poses = rows.shape[0] // case["K"]
    scores, matched, status = np.zeros(poses), np.zeros(poses, np.int32), np.zeros(4, np.int32)
    rc = h.frpbh_scores(*_orf(case["flags"]), case["P"], poses, case["K"], idx.shape[0], rows.ctypes.data, vis.ctypes.data, prior.ctypes.data,
                        idx.ctypes.data, case["lam"], criterion, scores.ctypes.data, matched.ctypes.data, status.ctypes.data)
    assert rc == 0
    return scores, matched, status


# the cases of the SCORE mode both test files run: (id, make_case arguments).  n = 1 .. 1000 over the workgroup edges at P = 1100 and
# 3 poses; K = 1, 2, 3, 6; all eight flag sets at n = 257
FULL = FLAG_SETS[-1]
SCORE_CASES = [(f"n{n}", dict(seed=100 + n, P=1100, poses=3, K=2, n=n, flags=FULL)) for n in (1, 63, 64, 65, 255, 256, 257, 1000)] + \
              [(f"K{K}", dict(seed=200 + K, P=1100, poses=3, K=K, n=300, flags=FULL)) for K in (1, 2, 3, 6)] + \
              [(f"flags-{flag_id(f)}", dict(seed=300 + i, P=1100, poses=3, K=2, n=257, flags=f)) for i, f in enumerate(FLAG_SETS)]
