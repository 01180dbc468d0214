"""popgs_term (csrc/fr_math.h), the per-entry term of fr_popgs_diag_criterion, compiled for the CPU: its branch logic against the
statement in its own comment, independently of the GPU's log1pf."""
import ctypes

import numpy as np
import pytest

C = np.float32(1e-12)            # FR_POPGS_CLAMP
F32 = np.float32


def _term(harness, dopt, ss, K, p, lam, c=C):
    ss, p = np.ascontiguousarray(ss, dtype=F32), np.ascontiguousarray(p, dtype=F32)
    assert ss.shape == p.shape and ss.ndim == 1
    term, J = np.empty_like(ss), np.empty_like(ss)
    fp = ctypes.POINTER(ctypes.c_float)
    f = harness.h_popgs_term
    f.restype = None
    f.argtypes = [ctypes.c_int, ctypes.c_int, fp, ctypes.c_int, fp, ctypes.c_float, ctypes.c_float, fp, fp]
    f(ss.size, int(dopt), ss.ctypes.data_as(fp), K, p.ctypes.data_as(fp), float(lam), float(c), term.ctypes.data_as(fp),
      J.ctypes.data_as(fp))
    return term, J


def _J(ss, K):
    """J as k_popgs_criterion forms it: ss * fl(1 / K) for a power of two (exact), ss / K otherwise."""
    return ss * (F32(1.0) / F32(K)) if K & (K - 1) == 0 else ss / F32(K)


def _grid(K, lam):
    """(ss, p) pairs: priors free and clamped, post below, on and above the clamp, J == 0, the quotient on either side of 3e38,
    and a log-uniform cloud over everything between."""
    lam, Kf = F32(lam), F32(K)
    ss, p = [], []

    def add(s, q):
        ss.append(F32(s)); p.append(F32(q))

    priors = [0.0, 1e-30, 1e-14, 4e-13, 9.99999e-13, np.nextafter(C, F32(0)), C, np.nextafter(C, F32(1)), 1.5e-12, 1e-9, 1e-3, 1.0, 37.5,
              1e4, 1e20]
    for q in priors:
        add(0.0, q)                                        # J == 0
        for s in (1e-30, 1e-14, 3e-13, 1e-12, 2.5e-12, 1e-6, 1.0, 3.0, 1e10, 1e27, 1e32, 3e38):
            add(s, q)
    # clamped prior, post on either side of c and equal to it: J = c - prior (exact by Sterbenz for prior >= c / 2), one ulp either way
    for q in (5e-13, 7.5e-13, 9e-13):
        pr = F32(q) + lam
        if pr < C:
            gap = C - pr
            for g in (np.nextafter(gap, F32(0)), gap, np.nextafter(gap, F32(1)), F32(0.5) * gap, F32(2) * gap):
                add(g * Kf, q)
    # the quotient around 3e38: d = 3e38 * base * (1 +- a few ulp .. 1 %), free (base = prior) and clamped (base = c)
    for q in (0.0, 3e-13, C, 1e-9, 1e-3, 0.25):
        base = max(F32(q) + lam, C)
        for f in (0.99, 0.9999, 1.0 - 2.0 ** -22, 1.0, 1.0 + 2.0 ** -22, 1.0001, 1.01, 1.1):
            s = np.float64(3e38) * np.float64(base) * f * K
            if s < 3.3e38:
                add(s, q)
    rng = np.random.default_rng(K)
    n = 4000
    cs = 10.0 ** rng.uniform(-20, 38, n)
    cp = 10.0 ** rng.uniform(-20, 20, n)
    cp[rng.random(n) < 0.2] = 0.0
    cs[rng.random(n) < 0.1] = 0.0
    return np.concatenate([np.array(ss, dtype=F32), cs.astype(F32)]), np.concatenate([np.array(p, dtype=F32), cp.astype(F32)])


@pytest.mark.parametrize("lam", [0.0, 1e-6, 0.1])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_topt_term_is_bit_equal(harness, K, lam):
    """1 / max(fl(fl(p + lam) + J), c), every operation a single IEEE binary32 one: the same bits as NumPy float32."""
    ss, p = _grid(K, lam)
    term, J = _term(harness, False, ss, K, p, lam)
    wantJ = _J(ss, K)
    assert wantJ.dtype == F32 and np.array_equal(J, wantJ)
    want = F32(1.0) / np.maximum((p + F32(lam)) + wantJ, C)
    assert want.dtype == F32 and np.array_equal(term, want)


@pytest.mark.parametrize("lam", [0.0, 1e-6, 0.1])
@pytest.mark.parametrize("K", [1, 3, 4])
def test_dopt_term_matches_its_statement(harness, K, lam):
    """log1p(d / base) in float64 on the function's own float32 intermediates: base = max(fl(p + lam), c), d = J where the prior is
    free, max(post, c) - c where it is clamped.  4 x 2^-24 relative: the quotient rounds once, log1pf is within 1 ulp, and beyond
    q = 3e38 the two logarithms are each within 1 ulp of a magnitude <= 90 against a difference >= 88.  Exactly 0.0 for J == 0 or
    post <= c -- the latter under a clamped prior, where d is formed from the rounded post; a free prior has post >= prior >= c, so
    post <= c means prior == c with J lost in the sum, and there the term is d / base = J / c as the statement has it (the true
    value, not 0).  Quotients below 2^-100 are left to the zero / sign checks: the bound is one of normal-range roundings."""
    ss, p = _grid(K, lam)
    term, J = _term(harness, True, ss, K, p, lam)
    assert np.array_equal(J, _J(ss, K))
    prior = p + F32(lam)
    post = prior + J
    assert prior.dtype == F32 and post.dtype == F32
    free = prior >= C
    base = np.where(free, prior, C)
    d = np.where(free, J, np.maximum(post, C) - C)
    assert d.dtype == F32 and base.dtype == F32
    q = d.astype(np.float64) / base.astype(np.float64)
    want = np.log1p(q)
    # the grid covers what it claims to
    clamped = ~free
    assert free.sum() > 100 and clamped.sum() > (100 if lam == 0.0 else -1)
    assert (J == 0).sum() > 10 and (q >= 3.0e38).sum() > 3 and ((q < 3.0e38) & (q > 2.9e38)).sum() > 0
    if lam == 0.0:
        assert (clamped & (post < C)).any() and (clamped & (post == C)).any() and (clamped & (post > C)).any()
        assert (clamped & (q >= 3.0e38)).any() and (free & (q >= 3.0e38)).any()
    zero = (J == 0) | (clamped & (post <= C))
    corner = free & (post <= C) & (J > 0)                  # prior == c exactly: held to the statement below, like every other term
    assert corner.any() == (lam == 0.0) and np.all(prior[corner] == C)
    assert np.all(term[zero] == 0.0) and np.all(want[zero] == 0.0)
    assert np.all(np.isfinite(term)) and np.all(term >= 0)
    zero |= q < 2.0 ** -100
    rel = np.abs(term.astype(np.float64) - want)[~zero] / want[~zero]
    far = q[~zero] >= 3.0e38
    print(f"\nK={K} lam={lam:g}: worst relative error {rel.max() * 2.0 ** 24:.2f} x 2^-24 over {rel.size} terms, "
          f"{(rel[far].max() * 2.0 ** 24 if far.any() else 0.0):.2f} x 2^-24 over the {int(far.sum())} beyond q = 3e38")
    assert rel.max() <= 4 * 2.0 ** -24, (rel.max() * 2.0 ** 24, ss[~zero][rel.argmax()], p[~zero][rel.argmax()])
