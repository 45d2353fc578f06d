"""Inputs of the register-copy claim re-sort's tests (test_sort_regs_model.py, test_sort_regs_gpu.py)."""
import random

import numpy as np

R = 3


def tables(n, r=R):
    """Per-claim template and headroom values no two claims share, the headroom beyond 32 bits."""
    ct = np.array([(c * 11 + 5) % 64 for c in range(n)], dtype=np.int32)
    ch = np.array([[(c << 33) + c * 1000003 + 19 * k - 7 for k in range(r)] for c in range(n)], dtype=np.int64).reshape(n, r)
    return ct, ch


def shuffled_order(n, seed=0):
    order = list(range(n))
    random.Random(seed * 7919 + n).shuffle(order)  # claim ids are not positions
    return order


def sample_positions(n):
    """0, n - 2 and the positions within one of choosePivot's samples: where the exact path is taken."""
    q = n // 4
    return sorted({p for p in [0, n - 2] + [s * q + d for s in (1, 2, 3) for d in (-1, 0, 1)] if 0 <= p < n})


def lifted(n):
    """The workload's own shape: non-decreasing with ties of width 1, 3 and 8, the entry at `pos` lifted by one and
    by more than the next block's width.  Yields (keys, pos)."""
    for w in (1, 3, 8):
        for lift in (1, w + 1):
            for pos in sample_positions(n):
                k = [i // w for i in range(n)]
                k[pos] += lift
                yield k, pos


def unbalanced(n):
    """The minimum everywhere but at every fifth position: choosePivot's median is the minimum, the first partition
    leaves nothing on its left, and the frame that continues on the right calls breakPatterns (from 14 entries on:
    what a first partition of 13 leaves is a leaf).  The lane model counts the calls; the tests assert them."""
    return [2 if i % 5 == 0 else 1 for i in range(n)]


def small_first(n, seed=0):
    """One small key, then larger random ones."""
    rng = random.Random(1000 + 31 * n + seed)
    return [0] + [rng.randint(1, 1000) for _ in range(n - 1)]
