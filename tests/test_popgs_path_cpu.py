"""POp-GS path evaluation (tester_gaussians_navigation.py:2109-2204), the parts that need no GPU: the round schedule, the
end-of-path rule, the layout conversion, and the argument validation of fr_popgs_diag_criterion."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from fisher_rast import _lib
    return _lib.load()


@pytest.mark.parametrize("acc", [4, 2])
def test_round_schedule_matches_literal_loop(acc):
    from fisher_rast.path_eval import popgs_round_schedule
    lengths = (9, 4, 3, 7, 0)
    want = {}                                            # path -> its accumulation steps, by the reference's own test (tester 2176)
    for i, n in enumerate(lengths):
        done = []
        for a in range(n):
            done.append(a)
            if (len(done) + 1) % acc == 0:
                want.setdefault(i, []).append(len(done))
    order, rounds = popgs_round_schedule(lengths, acc)
    assert sorted(order) == list(range(len(lengths)))
    got = {}
    for m, rnd in enumerate(rounds):
        assert rnd, "no empty round"
        # the active paths of a round are a prefix of `order`, in that order
        assert [i for i, _, _ in rnd] == order[:len(rnd)]
        for i, step, last in rnd:
            got.setdefault(i, []).append(step)
            assert len(got[i]) == m + 1                  # round m holds the path's m-th accumulation step
            assert last == (len(got[i]) == len(want[i]))
    assert got == want
    assert all(i in want or all(i != j for rnd in rounds for j, _, _ in rnd) for i in range(len(lengths)))
    if acc == 4:
        assert want == {0: [3, 7], 1: [3], 2: [3], 3: [3, 7]} and 4 not in got
    assert len(rounds) == max(len(v) for v in want.values())


def test_round_schedule_of_nothing():
    from fisher_rast.path_eval import popgs_round_schedule
    assert popgs_round_schedule([], 5) == ([], [])
    assert popgs_round_schedule([3, 0], 5)[1] == []
    with pytest.raises(ValueError):
        popgs_round_schedule([3], 0)


def test_end_of_path_rule():
    """tester 2186-2191: `path_end_weight` picks the branch, `object_path_end_weight` multiplies the final EIG."""
    from fisher_rast.path_eval import popgs_path_value
    terms, n, final = [-2.0, -0.5, 1.25], 7, 3.0
    assert popgs_path_value(terms, n, final, 0.0, 0.25) == (-1.25 + 3.0) / 7
    assert popgs_path_value(terms, n, final, 0.5, 0.25) == -1.25 / 7 + 0.25 * 3.0
    assert popgs_path_value(terms, n, final, 0.5, 0.0) == -1.25 / 7        # the tested weight is not the multiplier
    assert popgs_path_value([], 0, 2.0, 0.0, 9.0) == 2.0                    # no action: divides by max(len, 1)
    assert popgs_path_value([], 3, np.float32(1.5), 0.0, 0.0) == 0.5        # anything with .item()


def test_flat_layout_to_rows():
    import torch
    from fisher_rast.path_eval import popgs_rows_from_flat
    from models.SLAM.gaussian_object import ObjectFisherOps
    P = 5
    rows = torch.arange(P * 11, dtype=torch.float32).reshape(1, 1, P, 11).sqrt()
    flat = ObjectFisherOps._flat_diag(rows)[0]           # rows^2 in the reference's block order
    assert torch.equal(popgs_rows_from_flat(flat, P), (rows * rows)[0, 0])
    with pytest.raises(ValueError):
        popgs_rows_from_flat(flat[:-1], P)


def test_popgs_criterion_validates_without_gpu(lib):
    from fisher_rast import _lib
    q = lib.fr_popgs_diag_criterion_workspace_bytes
    assert int(q(0, 100)) == 0 and int(q(-3, 100)) == 0 and int(q(5, 0)) == 0
    E = 11 * 500000
    n = int(q(21, E))
    assert 21 * 8 <= n <= 21 * 8 * 4096 and n % (21 * 8) == 0
    assert int(q(1, E)) * 21 == n                         # the partials per view depend on E alone
    assert int(q(1, 3)) == 8
    fake = ctypes.c_void_p(1 << 20)                       # never dereferenced: every call below fails on the host
    f = lib.fr_popgs_diag_criterion

    def call(V=5, K=4, E=E, rows=fake, prior=fake, stride=0, out=None, acc=None, vis=None, lam=1e-6, crit=_lib.FR_POPGS_TOPT,
             scores=fake, ws=fake, ws_bytes=n):
        return f(V, K, E, rows, prior, stride, out, acc, vis, lam, crit, scores, ws, ws_bytes, None)

    assert call(rows=None) == _lib.FR_EINVAL and b"fr_popgs_diag_criterion" in lib.fr_last_error() and b"null" in lib.fr_last_error()
    assert call(scores=None) == _lib.FR_EINVAL
    assert call(prior=None) == _lib.FR_EINVAL
    assert call(V=0) == _lib.FR_EINVAL and call(V=-1) == _lib.FR_EINVAL
    assert call(K=0) == _lib.FR_EINVAL and call(K=-2) == _lib.FR_EINVAL
    assert call(E=0) == _lib.FR_EINVAL
    assert call(crit=2) == _lib.FR_EINVAL and b"criterion" in lib.fr_last_error()
    assert call(crit=-1) == _lib.FR_EINVAL
    assert call(stride=7) == _lib.FR_EINVAL
    assert call(lam=-1.0) == _lib.FR_EINVAL and call(lam=float("nan")) == _lib.FR_EINVAL
    assert call(ws_bytes=int(q(5, E)) - 1) == _lib.FR_ENOSPACE and b"workspace" in lib.fr_last_error()
    assert call(ws=None) == _lib.FR_ENOSPACE
    # a shared prior cannot be its own output when several views would write it
    assert call(out=fake, acc=fake, stride=0) == _lib.FR_EINVAL and b"overlaps" in lib.fr_last_error()


def test_ops_wrapper_refuses_cpu_tensors():
    import torch
    from fisher_rast import ops
    from fisher_rast._lib import FisherRastError
    with pytest.raises(FisherRastError):
        ops.popgs_diag_criterion(torch.zeros((2, 4, 3, 11)), torch.zeros((3, 11)))
