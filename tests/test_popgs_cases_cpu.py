"""tests/popgs_cases.py without a GPU: the float32 emulation of the criterion kernel's statements against the float64 restatement,
at the bounds the GPU tests put on the kernel, and the branch populations those tests rely on."""
import numpy as np
import pytest

import popgs_cases as pc

KS = (1, 2, 3, 4, 5, 7, 8)
LAMS = (0.0, 1e-6, 0.1)
ES = (1, 2, 3, 5, 1023, 1025, 1026, 98305)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_emulation_matches_restatement(family, E):
    """Scores within 1e-5 |want| and exactly 0 where want == 0, updated priors within (K + 3) 2^-24 want: the reference chain
    itself, rounded as the kernel rounds, meets the bounds of test_kernel_matches_float64_restatement on these families."""
    V = 3
    worst = (0.0, 0.0)
    for K in KS:
        for per_view in (False, True):
            rows, prior = pc.FAMILIES[family](V, K, E, seed=5, per_view=per_view)
            assert rows.shape == (V, K, E) and rows.dtype == np.float32 and prior.dtype == np.float32
            assert prior.shape == ((V, E) if per_view else (E,)) and np.all(np.isfinite(rows)) and np.all(prior >= 0)
            for lam in LAMS:
                for crit in ("topt", "dopt"):
                    s, out, _ = pc.emulate(rows, prior, lam, crit)
                    assert np.all(s <= 0) if crit == "topt" else np.all(s >= 0)
                    rel, ulp = pc.check(s, out, rows, prior, lam, crit, K, label=(family, E, K, per_view, lam, crit))
                    worst = (max(worst[0], rel), max(worst[1], ulp))
                    if crit == "dopt":
                        # the restatement against the two logarithms as written, at the latter's own rounding: per entry 2 roundings
                        # of 2^-53 |log| (|log| <= 76 over [1e-12, 1e33]) and post's, 2^-53 relative, on either logarithm's argument
                        lit = pc.restate(rows, prior, lam, crit, literal=True)[0]
                        assert np.all(np.abs(lit - pc.restate(rows, prior, lam, crit)[0]) <= E * (2 * 76 + 2) * 2.0 ** -53 + 1e-13 * lit)
    print(f"\n{family} E={E}: worst relative score error {worst[0]:.2e}, worst prior error {worst[1]:.2f} x 2^-24")


@pytest.mark.parametrize("E", [1023, 1025, 1026, 4099, 98305])
@pytest.mark.parametrize("K", [3, 4])
def test_branch_populations(E, K):
    """At lam = 0: `wide` puts at least 0.2 of its entries on the clamped prior, `far` at least 0.3 on the two-logarithm branch
    (0.33 and 0.50 by construction; a view of a handful of entries has no population to speak of, so E >= 1023 here)."""
    for per_view in (False, True):
        rows, prior = pc.wide(3, K, E, seed=5, per_view=per_view)
        sh = pc.emulate(rows, prior, 0.0, "dopt")[2]
        assert sh["clamped"] >= 0.2, sh
        assert np.mean(rows == 0) >= 0.4 and np.mean(np.all(rows == 0, axis=1)) >= 0.15      # 1 - 0.7 * 0.8 = 0.44; 0.2
        rows, prior = pc.far(3, K, E, seed=5, per_view=per_view)
        sh = pc.emulate(rows, prior, 0.0, "dopt")[2]
        assert sh["far"] >= 0.3 and sh["clamped"] >= 0.3, sh
        assert pc.emulate(rows, prior, 0.1, "dopt")[2]["far"] == 0.0                         # 1e32 / 0.1 stays inside fp32


def test_families_are_deterministic():
    for f in pc.FAMILIES.values():
        a, b = f(2, 3, 17, seed=1), f(2, 3, 17, seed=1)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert not np.array_equal(a[0], f(2, 3, 17, seed=2)[0])
