"""The plan of the register-resident key sort (csrc/fr_sortnet.h, compiled with g++ in tests/harness/fr_sortnet_harness.cpp) on the
CPU: the kernels' comparator lists, level conditions, partner rules and dispatch tables, run over a host model of 64 lanes x K
registers (one wave) and of four such runs joined (a workgroup), for every K = 1 .. 8 -- the powers of two the kernels have always
had and the K = 3, 5, 6, 7 that hold a run of n keys without padding it to the next power of two.

The in-lane lists are checked exhaustively by the zero-one principle (a comparator network sorts every input iff it sorts every
zero-one input; it sorts every bitonic input iff it sorts every bitonic zero-one input, a monotone map keeping a sequence bitonic);
whole runs are checked against std::sort inside the harness and against np.sort here."""
import ctypes

import numpy as np
import pytest

import harness_build

KS = list(range(1, 9))


@pytest.fixture(scope="module")
def net():
    h = ctypes.CDLL(harness_build.shared("fr_sortnet_harness", ()))
    h.frsn_sort_run.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32]
    for f in (h.frsn_list_len, h.frsn_list_failures):
        f.argtypes = [ctypes.c_int, ctypes.c_int]
    for f in (h.frsn_wave_k, h.frsn_wg4_k):
        f.argtypes = [ctypes.c_uint32]
    return h


def _run(net, K, nw, keys):
    """the plan's result for `keys` (a copy), after the harness's own comparison with std::sort"""
    k = np.ascontiguousarray(keys, np.uint64).copy()
    assert 0 < len(k) <= nw * 64 * K
    assert net.frsn_sort_run(K, nw, k.ctypes.data, len(k)) == 0, (K, nw, len(k))
    return k


@pytest.mark.parametrize("K", KS)
def test_in_lane_lists_by_the_zero_one_principle(net, K):
    """FrSnSort<K> sorts all 2^K zero-one inputs; FrSnClean<K> sorts every cyclically bitonic zero-one K-sequence (and, where it is
    shorter than a sorting network can be, is indeed no sorting network: the cheaper list is in use)."""
    assert net.frsn_list_failures(K, 0) == 0
    assert net.frsn_list_failures(K, 1) == 0
    optimal = {1: 0, 2: 1, 3: 3, 4: 5, 5: 9, 6: 12, 7: 16, 8: 19}          # fewest comparators of a sorting network (Knuth 5.3.4)
    assert net.frsn_list_len(K, 0) >= optimal[K]
    if K not in (1, 2, 4, 8):
        assert net.frsn_list_len(K, 0) == optimal[K]
    assert net.frsn_list_len(K, 1) <= net.frsn_list_len(K, 0)


def _inputs(rng, n):
    """(name, keys): random, heavy ties, all equal, ascending, descending, organ pipe, and keys that already are the padding value"""
    asc = np.arange(n, dtype=np.uint64) * np.uint64(3) + np.uint64(5)
    half = (n + 1) // 2
    organ = np.concatenate([asc[:half], asc[:n - half][::-1]])
    top = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    top[rng.random(n) < 0.2] = np.uint64(0xFFFFFFFFFFFFFFFF)
    return [("random", rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)),
            ("ties", rng.integers(0, 5, n, dtype=np.uint64)),
            ("equal", np.full(n, 77, np.uint64)),
            ("ascending", asc), ("descending", asc[::-1].copy()), ("organ pipe", organ), ("with ~0 keys", top)]


def _lengths(K, nw, rng):
    """full, one short of full, one beyond the next smaller K, one beyond half (a level more), tiny, and a few at random"""
    cap = nw * 64 * K
    fixed = {cap, cap - 1, max(2, nw * 64 * (K - 1) + 1), cap // 2 + 1, cap // 2, 2, 3, 65}
    return sorted({n for n in fixed if 1 < n <= cap} | {int(x) for x in rng.integers(2, cap + 1, 6)})


@pytest.mark.parametrize("nw", [1, 4])
@pytest.mark.parametrize("K", KS)
def test_whole_runs_equal_a_sort(net, K, nw):
    """one wave (nw = 1) and four waves joined (nw = 4): full runs and runs of n < nw 64 K keys padded with ~0"""
    rng = np.random.default_rng(100 * K + nw)
    for n in _lengths(K, nw, rng):
        for name, keys in _inputs(rng, n):
            got = _run(net, K, nw, keys)
            assert np.array_equal(got, np.sort(keys)), (K, nw, n, name)


def test_random_lengths_with_ties_and_padding(net):
    """300 lengths per K for one wave (the check the network's argument was first made with), 60 per K for four waves"""
    rng = np.random.default_rng(7)
    for K in KS:
        for nw, trials in ((1, 300), (4, 60)):
            for n in rng.integers(1, nw * 64 * K + 1, trials):
                keys = rng.integers(0, 1 + int(n) // 3, int(n), dtype=np.uint64)
                assert np.array_equal(_run(net, K, nw, keys), np.sort(keys)), (K, nw, int(n))


def test_dispatch_takes_the_smallest_instantiated_run(net):
    """fr_sn_wave_k / fr_sn_wg4_k: an instantiated K (the masks' bits), large enough for n, and no instantiated K below it is"""
    for per, fn, mask, lo, hi in ((64, net.frsn_wave_k, net.frsn_wave_ks(), 2, 512), (256, net.frsn_wg4_k, net.frsn_wg4_ks(), 513, 2048)):
        have = [K for K in range(1, 8) if (mask >> K) & 1] + [8]
        for n in range(lo, hi + 1):
            K = fn(n)
            assert K in have and per * K >= n, (n, K)
            assert all(per * k < n for k in have if k < K), (n, K)
    # the instantiated runs: every K for one wave, 3 .. 8 for four
    assert net.frsn_wave_ks() == 0x1FE and net.frsn_wg4_ks() == 0x1F8
