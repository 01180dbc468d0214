"""-m gpu: the register-resident key sort with any number of keys per lane.  A list or a part of n keys is held by one wave with
K = ceil(n / 64) keys per lane (n <= 512) or by four waves with K = ceil(n / 256) (513 .. 2048), K no longer a power of two
(csrc/fr_sortnet.h; tests/test_sortnet_cpu.py checks the plan itself on the CPU).

Short lists: the method of tests/test_gpu_sort_sizes.py (one tile takes every splat, tied depths, expected keys computed on the
host) at the lengths on both sides of every change of K.  Parts: the 128-list scene of test_gpu_sort_items.py's
test_parts_beyond_one_wave, whose ~8000 parts spread over every class ceil(c / 64) = 1 .. 8; the partition is replayed on the host
and the presence of every class is asserted as a condition on the input."""
import numpy as np
import pytest
import torch

from test_gpu_sort_items import (SMALL_MAX, _cam, _check_segments_and_parts, _many_lists_scene, _part_max, _poses, _read_back,
                                 _replay_partition, _scorer)
from test_gpu_sort_sizes import _check

pytestmark = pytest.mark.gpu

# one wave: K changes at 64 K (3 .. 7); four waves: at 256 K (3 .. 7)
EDGES = [191, 192, 193, 319, 320, 321, 383, 384, 385, 447, 448, 449, 767, 768, 769, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793]


@pytest.mark.parametrize("n", EDGES)
def test_short_list_where_the_keys_per_lane_change(gpu, oracle, n):
    _check(gpu, oracle, n)


@pytest.mark.parametrize("n", [320, 768, 1280, 1536])
def test_short_list_of_three_depths(gpu, oracle, n):
    """3 distinct depth values: long runs of equal depth, ordered by the index alone"""
    _check(gpu, oracle, n, 3)


def test_parts_of_every_size_class(gpu):
    """Lists of 16000 .. 16320 keys, NP = 64: part sizes spread like a Gamma(8) variable around 250, so k_sort_parts meets parts of
    every class ceil(c / 64) = 1 .. 8 (the rarest, up to 64 keys, about 9 times in 8000).  Every segment must come out strictly
    ascending and a permutation of the unsorted list that still stands at the segment's start."""
    V, capacity = 2, 32768
    W, H, args = _many_lists_scene(gpu, seed=21, heavy_lo=16000, heavy_hi=16321, all_heavy=True)
    P = args[0].shape[0]
    sc = _scorer(args, _cam(W, H, gpu), capacity)
    Hi = (torch.rand((P, 4), generator=torch.Generator().manual_seed(1)) + 0.05).to(gpu)
    sc.run(_poses(gpu, V, step=0.002), H_inv=Hi)
    assert sc.tile_capacity == capacity
    cnt, toff, keys, n_parts, desc = _read_back(sc, P, W, H, V)
    classes = np.zeros(10, np.int64)
    n_long = 0
    for i in range(len(cnt)):
        n = int(cnt[i])
        seg = keys[toff[i]:toff[i] + n]
        assert np.all(seg[1:] > seg[:-1]), (i, n)
        if not (SMALL_MAX < n <= _part_max(capacity)):
            continue
        n_long += 1
        unsorted = keys[i * capacity:i * capacity + n]
        assert np.array_equal(np.sort(unsorted), seg), (i, n)
        sizes = _replay_partition(unsorted)
        sizes = sizes[(sizes >= 2) & (sizes <= 512)]                  # the parts k_sort_parts is given
        classes += np.bincount((sizes + 63) // 64, minlength=10)
    _check_segments_and_parts(cnt, toff, keys, n_parts, desc, capacity)        # the part list itself, entry by entry
    print(f"{n_long} lists, {n_parts} parts; parts per class ceil(c / 64) = 1 .. 8: {classes[1:9].tolist()}")
    assert n_long == 64 * V
    # a condition on the input, not a result: without it the test would pass for nothing
    assert (classes[1:9] >= 1).all(), f"the scene has no part in some size class: {classes[1:9].tolist()}"
