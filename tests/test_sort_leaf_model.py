"""The exact claim re-sort's leaves (ks_solve.hip ClaimSort::w_leaf, KS_SORT_LEAF).

pdqsort_func sorts a frame of at most 12 entries with insertionSort_func (src/sort/zsortfunc.go), which only ever
exchanges an entry with a strictly greater left neighbour: it is a stable sort.  The kernel therefore places the
frame in one step: lane i counts the entries that sort before its own,
rank(i) = #{j : key[j] < key[i] or (key[j] == key[i] and j < i)}, and stores its (key, payload) at a + rank(i).

Checked here against a model of Go's loop itself, on the payloads (which entry went where), not only the keys."""
import itertools
import random

from test_sort_single_descent import Data


def go_insertion_sort(data, a, b):
    """insertionSort_func."""
    for i in range(a + 1, b):
        j = i
        while j > a and data.less(j, j - 1):
            data.swap(j, j - 1)
            j -= 1


def stable_rank_leaf(pairs, a, b):
    """The kernel's leaf on [a, b): every lane reads its entry and the frame's keys, then all store at once."""
    d = list(pairs)
    n = b - a
    assert n <= 12
    keys = [d[a + j][0] for j in range(n)]
    rank = [sum(1 for j in range(n) if keys[j] < keys[i] or (keys[j] == keys[i] and j < i)) for i in range(n)]
    assert sorted(rank) == list(range(n))  # a permutation: the stores do not collide
    out = list(d)
    for i in range(n):
        out[a + rank[i]] = d[a + i]
    return out


def check(keys, a=0, pad=0):
    """The frame [a, a + len(keys)) inside an array with `pad` entries on both sides that must stay put."""
    n = len(keys)
    pairs = [(99 - i, 1000 + i) for i in range(pad)] + [(k, i) for i, k in enumerate(keys)] + \
            [(-5 - i, 2000 + i) for i in range(pad)]
    data = Data(pairs)
    go_insertion_sort(data, a + pad, a + pad + n)
    got = stable_rank_leaf(pairs, a + pad, a + pad + n)
    assert got == data.d, (keys, got, data.d)  # the same permutation of the indices
    assert got[:pad] == pairs[:pad] and got[pad + n:] == pairs[pad + n:]


def test_exhaustive_up_to_seven_entries_over_three_key_values():
    cases = 0
    for n in range(0, 8):
        for keys in itertools.product((1, 2, 3), repeat=n):
            check(list(keys))
            cases += 1
    assert cases == sum(3 ** n for n in range(8))


def test_random_frames_of_eight_to_twelve_entries():
    rng = random.Random(11)
    for case in range(2000):
        n = rng.randint(8, 12)
        vals = rng.randint(1, 4)
        check([rng.randint(1, vals) for _ in range(n)], pad=case % 3)


def test_the_leaf_is_go_for_every_length_on_the_two_extremes():
    for n in range(0, 13):
        check(list(range(n, 0, -1)), pad=2)  # reversed: the most exchanges
        check([7] * n, pad=2)  # all equal: none
