"""Synthetic probe rows and priors for fr_popgs_diag_criterion (csrc/fr_popgs.hip), its float64 restatement, and a NumPy float32
emulation of the kernel's statements.  The rows of a real probe launch have E = 11 P entries, a few zeros and magnitudes a render
produces; the families here put the kernel where such rows never do: any E, zeros by element and by column, priors on either side
of the clamp, quotients beyond fp32.  Helper module of tests/test_popgs_cases_cpu.py (which holds `emulate` to `restate` and
checks that each family has the branch population it is named for), tests/test_gpu_popgs_synthetic.py and
tests/test_gpu_popgs_path.py.
"""
import numpy as np

CLAMP = 1e-12            # FR_POPGS_CLAMP (include/fisher_rast.h)
FAR_Q = 3.0e38           # popgs_term takes two logarithms from this quotient on


def restate(rows, prior, lam, crit, literal=False):
    """float64 NumPy on the float32 inputs: J, scores [V], prior + J.  rows [V,K,E], prior [E] or [V,E].
    D-opt is log max(post, c) - log max(prior, c) written as log1p((max(post, c) - max(prior, c)) / max(prior, c)), the numerator
    being J under a free prior.  `literal` gives the difference of the two float64 logarithms as written: each is rounded at
    2^-53 of a magnitude up to 32, an absolute 7e-15 per entry, which is more than 1e-5 of the score of a view that has a handful
    of entries with J / prior < 1e-9 (wide, E = 2: 4.5e-5 off) and nothing next to 33 000 entries of a render.
    tests/test_popgs_cases_cpu.py holds the two forms together at that absolute bound."""
    r = rows.astype(np.float64)
    J = (r * r).sum(axis=1) / r.shape[1]
    pin = np.broadcast_to(prior.astype(np.float64), J.shape)
    pr = pin + np.float64(np.float32(lam))                 # lam as the ABI carries it
    post = pr + J
    if crit == "topt":
        s = -(1.0 / np.maximum(post, CLAMP)).sum(axis=1)
    elif literal:
        s = (np.log(np.maximum(post, CLAMP)) - np.log(np.maximum(pr, CLAMP))).sum(axis=1)
    else:
        base = np.maximum(pr, CLAMP)
        s = np.log1p(np.where(pr >= CLAMP, J, np.maximum(post, CLAMP) - CLAMP) / base).sum(axis=1)
    return s, pin + J


def _log_uniform(rng, lo, hi, shape):
    return 10.0 ** rng.uniform(lo, hi, size=shape)


def _prior_shape(V, E, per_view):
    return (V, E) if per_view else (E,)


def wide(V, K, E, seed, per_view=False):
    """Row magnitudes log-uniform in [1e-6, 1e2] with random signs, 30 % of the elements zero and 20 % of the columns (v, e) zero
    over all K probes (J == 0); prior log-uniform in [1e-14, 1e4] with 25 % exact zeros.  Returns float32 rows [V,K,E], prior."""
    rng = np.random.default_rng([seed, V, K, E, int(per_view), 1])
    rows = _log_uniform(rng, -6.0, 2.0, (V, K, E)) * rng.choice([-1.0, 1.0], size=(V, K, E))
    rows[rng.random((V, K, E)) < 0.3] = 0.0
    rows *= (rng.random((V, 1, E)) >= 0.2)
    prior = _log_uniform(rng, -14.0, 4.0, _prior_shape(V, E, per_view))
    prior[rng.random(prior.shape) < 0.25] = 0.0
    return rows.astype(np.float32), prior.astype(np.float32)


def far(V, K, E, seed, per_view=False):
    """On half of the entries e (the same for every view) row magnitudes log-uniform in [1e14, 1e16] under a prior of 0 (half of
    them) or log-uniform in [1e-14, 10^-12.5]: J >= 1e28 over a base of 1e-12 at lam = 0, a quotient beyond fp32.  The other entries
    are ordinary: rows in [1e-3, 1e1], prior in [1e-3, 1e2].  Random signs.  Returns float32 rows [V,K,E], prior."""
    rng = np.random.default_rng([seed, V, K, E, int(per_view), 2])
    big = rng.random(E) < 0.5
    mag = np.where(big, _log_uniform(rng, 14.0, 16.0, (V, K, E)), _log_uniform(rng, -3.0, 1.0, (V, K, E)))
    rows = mag * rng.choice([-1.0, 1.0], size=(V, K, E))
    shape = _prior_shape(V, E, per_view)
    tiny = _log_uniform(rng, -14.0, -12.5, shape)
    tiny[rng.random(shape) < 0.5] = 0.0
    prior = np.where(big, tiny, _log_uniform(rng, -3.0, 2.0, shape))
    return rows.astype(np.float32), prior.astype(np.float32)


FAMILIES = {"wide": wide, "far": far}


def emulate(rows, prior, lam, crit):
    """The kernel's statements in NumPy float32: ss by one rounding per probe (fmaf), J = ss * (1/K) for a power of two and ss / K
    otherwise, prior = p + lam, post = prior + J, the term with its branches (popgs_term), the terms added in float64.  Returns
    (scores [V] float64, prior + J [V,E] float32, shares) with shares = the fractions of all (v, e) on the D-opt term's branches:
    `clamped` (p + lam < 1e-12) and `far` (d / base >= 3e38)."""
    f32 = np.float32
    r = np.asarray(rows, dtype=f32)
    V, K, E = r.shape
    ss = np.zeros((V, E), dtype=f32)
    for k in range(K):
        x = r[:, k].astype(np.float64)
        ss = (x * x + ss.astype(np.float64)).astype(f32)     # x * x is exact in float64: one rounding (twice, rarely) per probe
    J = ss * (f32(1.0) / f32(K)) if K & (K - 1) == 0 else ss / f32(K)
    p = np.broadcast_to(np.asarray(prior, dtype=f32), (V, E))
    c = f32(CLAMP)
    pr = p + f32(lam)
    post = pr + J
    free = pr >= c
    base = np.where(free, pr, c)
    d = np.where(free, J, np.maximum(post, c) - c)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        q = d / base                                       # float32: overflows to inf, which is >= 3e38
        is_far = ~(q < f32(FAR_Q))
        if crit == "topt":
            term = f32(1.0) / np.maximum(post, c)
        else:
            term = np.where(is_far, np.log(d) - np.log(base), np.log1p(np.where(is_far, f32(0.0), q)))
    assert J.dtype == f32 and term.dtype == f32 and post.dtype == f32
    s = term.astype(np.float64).sum(axis=1)
    shares = {"clamped": float(np.mean(~free)), "far": float(np.mean(is_far))}
    return (-s if crit == "topt" else s), p + J, shares


def check(got_scores, got_prior, rows, prior, lam, crit, K, views=None, label=""):
    """The two bounds of test_kernel_matches_float64_restatement against `restate`: scores within 1e-5 |want| and exactly 0 where
    want == 0; written priors within (K + 3) 2^-24 want (`views` = the views whose block was written; all when None).  Returns
    (worst relative score error, worst prior error in units of 2^-24 want)."""
    want, want_prior = restate(rows, prior, lam, crit)
    got = np.asarray(got_scores, dtype=np.float64)
    assert np.all(np.isfinite(got)), (label, got)
    assert np.all(got[want == 0] == 0.0), (label, got, want)
    assert np.all(np.abs(got - want) <= 1e-5 * np.abs(want)), (label, got, want)
    nz = want != 0
    rel = float((np.abs(got - want)[nz] / np.abs(want[nz])).max()) if nz.any() else 0.0
    worst_p = 0.0
    if got_prior is not None:
        o = np.asarray(got_prior).astype(np.float64)
        for v in (range(o.shape[0]) if views is None else views):
            err = np.abs(o[v] - want_prior[v])
            bad = err > (K + 3) * 2.0 ** -24 * want_prior[v]
            assert not bad.any(), (label, v, int(bad.sum()), o[v][bad][:4], want_prior[v][bad][:4])
            pos = want_prior[v] > 0
            if pos.any():
                worst_p = max(worst_p, float((err[pos] / want_prior[v][pos]).max() * 2.0 ** 24))
    return rel, worst_p
