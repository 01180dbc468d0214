"""The table of tests/stream_cases.py without a GPU: `real` and `decoy` of every case agree in names, shapes, dtypes and contiguity
(the stream-ordered run overwrites one with the other in place), every index input lies within its bounds (a wrong-stream bug must
show as a wrong number, never as an access out of bounds), and the two differ wherever the case does not keep them equal on
purpose."""
import numpy as np
import pytest

import stream_cases as sc


@pytest.fixture(scope="module", params=sc.names())
def pair(request):
    case = sc.by_name(request.param)
    return case, case.make(0), case.make(1)


def test_real_and_decoy_have_one_layout(pair):
    case, real, decoy = pair
    assert list(real) == list(decoy), case.name
    for k, r in real.items():
        d = decoy[k]
        assert isinstance(r, np.ndarray) and isinstance(d, np.ndarray), (case.name, k)
        assert r.shape == d.shape and r.dtype == d.dtype, (case.name, k, r.shape, d.shape, r.dtype, d.dtype)
        assert r.flags["C_CONTIGUOUS"] and d.flags["C_CONTIGUOUS"], (case.name, k)
        assert r.dtype in (np.float32, np.int32, np.int64, np.uint8), (case.name, k, r.dtype)
        if r.dtype == np.float32:
            assert np.isfinite(r).all() and np.isfinite(d).all(), (case.name, k)


def test_index_inputs_are_within_their_bounds(pair):
    case, real, decoy = pair
    integer = {k for k, v in real.items() if v.dtype in (np.int32, np.int64)}
    # every integer input is an index or a count the kernels act on: each needs a stated range (uint8 inputs are masks and flags)
    assert integer <= set(case.bounds), (case.name, integer - set(case.bounds))
    for k, (lo, hi) in case.bounds.items():
        for a in (real[k], decoy[k]):
            assert a.size and lo <= int(a.min()) and int(a.max()) < hi, (case.name, k, int(a.min()), int(a.max()), lo, hi)
    for k, v in real.items():
        if v.dtype == np.uint8:
            assert int(v.max()) <= 1 and int(decoy[k].max()) <= 1, (case.name, k)


def test_real_and_decoy_differ(pair):
    case, real, decoy = pair
    assert set(case.same) <= set(real), (case.name, set(case.same) - set(real))
    varied = [k for k in real if k not in case.same]
    assert varied, case.name
    for k in varied:
        assert not np.array_equal(real[k], decoy[k]), f"{case.name}: {k} is the same in real and decoy"
    for k in case.same:
        assert np.array_equal(real[k], decoy[k]), f"{case.name}: {k} is listed as kept equal and differs"


def test_every_case_compares_something_and_names_its_rule():
    seen = set()
    for case in sc.cases():
        assert case.name not in seen
        seen.add(case.name)
        assert case.exact or case.close, case.name
        assert not (set(case.exact) & set(case.close)), case.name
        assert bool(case.close) == bool(case.close_from), f"{case.name}: a tolerance is quoted from an existing parity test, by name"
    assert sc.BLOCKER_MS >= 20.0 and sc.BLOCKER_MS <= sc.BLOCKER_CAP_MS == 250.0
