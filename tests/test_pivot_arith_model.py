"""choosePivot's hint and pivot by arithmetic (KS_PIVOT_ARITH) and the appended claim's closed form, on the Go model
of tests/test_sort_single_descent.py.

Every descent the LEAN Solve leaves in s.newNodeClaims has a known origin.

  A count crossing at `pos`: a run's segment lifts key[pos] to key[pos+1] + 1 (a single pod: a tie lifted by one),
  the array is non-decreasing but for key[pos] > key[pos+1].  For n >= 50 choosePivot_func reads the triples
  {l-1, l, l+1}, {2l-1, 2l, 2l+1}, {3l-1, 3l, 3l+1}, l = n/4.  Its hint is "increasing" exactly when pos is none of
  l-1, l, 2l-1, 2l, 3l-1, 3l (the descent then lies inside no triple), and its pivot is then 2l.  The kernel takes
  that from n and pos alone once it has confirmed the descent; on the six positions, below 50 entries and without a
  descent at pos it samples as before.

  An appended claim: non-decreasing on [0, n-1), key[n-1] < key[n-2].  For n >= 50 the samples end at
  3l + 1 < n - 1: the hint is "increasing", partialInsertionSort swaps the last pair, walks the new entry left past
  every greater key and finds no second descent: with p = #{q < n-1 : key[q] <= key[n-1]}, [p, n-1) moves one place
  right and the new entry lands at p.

All of this is condition against model, no measurement."""
import random

from test_sort_single_descent import Data, go_choose_pivot, go_top_frame

WAVE = 64


class Keys:
    """Keys alone behind Go's less (choosePivot_func reads, never swaps)."""

    def __init__(self, keys):
        self.k = keys

    def less(self, i, j):
        return self.k[i] < self.k[j]


def sample_positions(n):
    """The six positions whose pair (pos, pos + 1) lies inside one of choosePivot's triples (n >= 50)."""
    l = n // 4
    return {l - 1, l, 2 * l - 1, 2 * l, 3 * l - 1, 3 * l}


def arith(keys, pos):
    """The kernel's arithmetic form: (hint, pivot), or None where it samples as before."""
    n = len(keys)
    if n < 50 or pos < 0 or pos + 1 >= n or not keys[pos] > keys[pos + 1]:
        return None
    l = n // 4
    e = pos - (l - 1)  # as ClaimSort::pivot_sampled tests it
    if e in (0, 1, l, l + 1, 2 * l, 2 * l + 1):
        return None
    return 1, 2 * l


def cells(n):
    l = n // 4
    c = {0, n - 2}
    for m in (l, 2 * l, 3 * l):
        c |= {m - 2, m - 1, m, m + 1}
    return sorted(c)


def crossed(keys, pos):
    """The array a run's segment leaves: the claim at pos lifted to one past its right neighbour's count."""
    k = list(keys)
    k[pos] = k[pos + 1] + 1
    return k


def tied(n, width, rng):
    if width == 0:  # all distinct
        return [2 * i for i in range(n)]
    return sorted(rng.randint(1, 1 + max(1, n // width // 4)) for _ in range(n))


def check_crossing(k, pos, tally):
    n = len(k)
    pivot, hint = go_choose_pivot(Keys(k), 0, n)
    got = arith(k, pos)
    six = pos in sample_positions(n)
    # conditions: outside the six the arithmetic form must decide, on the six it must not
    assert (got is not None) == (not six), (n, pos, got)
    assert (hint == 1) == (not six), (n, pos, hint)
    if got is not None:
        assert got == (hint, pivot), (n, pos, got, hint, pivot)
        tally[1] += 1
    tally[0] += 1


def test_every_single_crossing_against_choose_pivot():
    rng = random.Random(17)
    tally = [0, 0]
    for n in list(range(50, 301)) + [1023, 1024]:
        for width in (1, 3, 12, 0):
            keys = tied(n, width, rng)
            for pos in range(n - 1):
                check_crossing(crossed(keys, pos), pos, tally)
    print("arrays %d, decided by arithmetic %d" % tuple(tally))
    assert tally[0] > 150000 and tally[0] - tally[1] == 6 * 4 * (251 + 2)


def test_cells_around_the_samples_for_every_n_mod_4():
    seen = set()
    for n in (50, 51, 52, 53, 64, 65, 66, 67, 122, 129, 257, 321, 1023, 1024):
        seen.add(n % 4)
        tally = [0, 0]
        for base in ([5] * n, [i // 3 for i in range(n)], [2 * i for i in range(n)]):
            for pos in cells(n):
                check_crossing(crossed(base, pos), pos, tally)
        assert tally[0] - tally[1] == 6 * 3, (n, tally)
    assert seen == {0, 1, 2, 3}


def append_closed(pairs):
    """The appended claim's closed form as the kernel runs it, or None where it refuses: p by ballots over 64-entry
    chunks that stop at the first chunk holding a greater key, [p, n-1) one place right in chunks, high chunk first,
    each read whole before it is written, the new entry at p.  Returns (array, tlo, thi)."""
    d = list(pairs)
    n = len(d)
    if n < 50 or not d[n - 1][0] < d[n - 2][0]:
        return None
    new = d[n - 1]
    p = 0
    for base in range(0, n - 1, WAVE):
        le = [q < n - 1 and d[q][0] <= new[0] for q in range(base, base + WAVE)]
        p += sum(le)
        if not all(le):
            break
    for hi in range(n - 1, p, -WAVE):
        lo = max(hi - WAVE, p)
        chunk = [d[j] for j in range(lo, hi)]
        for j, e in zip(range(lo, hi), chunk):
            d[j + 1] = e
    d[p] = new
    return d, p, n - 1


def check_append(keys, new):
    pairs = [(k, i) for i, k in enumerate(keys)] + [(new, len(keys))]
    n = len(pairs)
    finished, hint, want = go_top_frame(pairs)
    assert hint == 1 and finished, (n, new)
    got, tlo, thi = append_closed(pairs)
    assert got == want, (n, new, tlo)
    assert tlo == sum(k <= new for k in keys) and thi == n - 1
    assert [i for i in range(n) if pairs[i] != want[i]] == list(range(tlo, n))
    return tlo


def test_appended_claim_against_go_top_frame():
    rng = random.Random(23)
    cases = 0
    for n in range(50, 300):
        for rep in range(12):
            width = (1, 3, 12, 0)[rep % 4]
            keys = tied(n - 1, width, rng)
            new = rng.randint(keys[0] - 1, keys[-1] - 1)
            check_append(keys, new)
            cases += 1
    assert cases == 3000
    for n in (50, 64, 65, 129, 130, 257, 1024):
        # no key equal to the new one, one, many; p = 0 and p = n - 2 among them
        assert check_append([3] * (n - 1), 1) == 0
        assert check_append([1] + [3] * (n - 2), 1) == 1
        assert check_append([1] * (n - 2) + [3], 1) == n - 2
        assert check_append([1] * (n // 2) + [2] * (n - 1 - n // 2), 1) == n // 2
        assert check_append(list(range(n - 1)), n - 3) == n - 2
        assert check_append([0] * 70 + [5] * (n - 71) if n > 80 else [0] * 40 + [5] * (n - 41), 4) == (70 if n > 80 else 40)


def test_the_refusals():
    """Below 50 entries, without a descent at pos, and with a new entry not below its neighbour the kernel runs as
    before; the model shows why each is not the closed forms'."""
    k49 = crossed([5] * 49, 10)
    assert arith(k49, 10) is None
    finished, _, d = go_top_frame([(k, i) for i, k in enumerate(k49)])
    assert not finished and [x[0] for x in d] == k49  # the frame hands the array on untouched
    flat = [i // 3 for i in range(90)]
    assert arith(flat, 10) is None and arith(flat, -1) is None and arith(flat, 89) is None
    assert arith(crossed(flat, 10), 11) is None  # a descent, but not at pos
    assert arith(crossed(flat, 10), 10) == (1, 44)
    assert append_closed([(k, i) for i, k in enumerate([5] * 48 + [1])]) is None  # n = 49
    assert append_closed([(k, i) for i, k in enumerate([1] * 60)]) is None  # key[n-1] == key[n-2]
    assert append_closed([(k, i) for i, k in enumerate([1] * 59 + [2])]) is None  # key[n-1] > key[n-2]
    # on a sample position the sampled hint is not "increasing": the general path's pivot is the sampled one
    k = crossed([5] * 64, 16)
    assert arith(k, 16) is None and go_choose_pivot(Data([(x, i) for i, x in enumerate(k)]), 0, 64)[1] == 0
