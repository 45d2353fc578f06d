"""ks_claim_sort_probe's host mode (device -1: Go's pdqsort_func of csrc/ks_gosort.h, the expected value of
tests/test_sort_probe_gpu.py) checked without a GPU: it sorts, keeps the pairs together, regathers the position
arrays, equals the stable order on the leaves (<= 12 entries: insertionSort_func), leaves a non-decreasing array
alone, and refuses arguments the kernel could not take."""
import random

import numpy as np
import pytest

from karpenter_amd import KsError, claim_sort_probe


def tables(n, r):
    ct = np.array([(c * 5 + 1) % 64 for c in range(n)], dtype=np.int32)
    ch = np.array([[(c << 34) - 3 * c + k for k in range(r)] for c in range(n)], dtype=np.int64).reshape(n, r)
    return ct, ch


@pytest.mark.parametrize("r", (3, 4))
def test_host_mode_sorts_pairs_and_regathers(r):
    rng = random.Random(5)
    for n in (0, 1, 2, 12, 13, 49, 50, 64, 65, 300, 1024):
        keys = [rng.randint(1, max(n // 3, 1)) for _ in range(n)]
        order = list(range(n))
        rng.shuffle(order)
        ct, ch = tables(n, r)
        k, o, pt, ph, how = claim_sort_probe(keys, order, ct, ch, device=-1)
        assert how == 1 and list(k) == sorted(keys)
        assert sorted(zip(k.tolist(), o.tolist())) == sorted(zip(keys, order))  # the pairs stayed together
        assert np.array_equal(pt, ct[o]) and np.array_equal(ph, ch[o].reshape(n, r))
        if n <= 12:  # insertionSort_func is stable
            assert list(zip(k.tolist(), o.tolist())) == sorted(zip(keys, order), key=lambda e: e[0])
        again = claim_sort_probe(k, o, ct, ch, device=-1)
        assert list(again[1]) == list(o)  # pdqsort leaves a non-decreasing array untouched


def test_arguments_are_checked():
    ct, ch = tables(4, 3)
    ok = ([1, 2, 3, 4], [0, 1, 2, 3], ct, ch)
    claim_sort_probe(*ok, device=-1)
    for bad in (dict(mode=2), dict(mode=1, pos=4), dict(mode=1, pos=-1)):
        with pytest.raises(KsError):
            claim_sort_probe(*ok, device=-1, **bad)
    with pytest.raises(KsError):
        claim_sort_probe([1, 2, 3, 4], [0, 1, 2, 4], ct, ch, device=-1)  # not a claim id
    with pytest.raises(KsError):
        claim_sort_probe([1, 2, 3, 4], [0, 1, 2, 3], ct, np.zeros((4, 5), dtype=np.int64), device=-1)  # R
    big = 1025
    with pytest.raises(KsError):
        claim_sort_probe([1] * big, list(range(big)), *tables(big, 3), device=-1)
