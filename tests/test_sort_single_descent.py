"""The LEAN Solve's closed-form claim re-sort (ks_solve.hip sort_single_descent, KS_SORT_CLOSED).

Every descent the LEAN Solve leaves in s.newNodeClaims comes from one increment of one claim's pod count at a
known sorted position `pos`: the array is non-decreasing except key[pos] > key[pos+1].  For n >= 50 and
choosePivot's hint "increasing", Go 1.21's pdqsort_func (src/sort/zsortfunc.go, the sort.Slice that
scheduler.go:247 calls) finishes inside partialInsertionSort_func, and its effect is: with
t = #{q in (pos, n): key[q] < key[pos]}, the entries pos+1 .. pos+t move one place left in order, the claim
lands at pos + t, nothing else moves.

Checked here against a model of the Go loops themselves (choosePivot_func and partialInsertionSort_func of the
top-level frame), payloads included so the tie order is compared too.  The closed form is written as the
kernel runs it: the count by 64-lane ballots, the shift in 64-entry chunks each read before it is written."""
import random

WAVE = 64


class Data:
    """(key, payload) pairs behind Go's lessSwap."""

    def __init__(self, pairs):
        self.d = list(pairs)

    def less(self, i, j):
        return self.d[i][0] < self.d[j][0]

    def swap(self, i, j):
        self.d[i], self.d[j] = self.d[j], self.d[i]


def go_choose_pivot(data, a, b):
    """choosePivot_func: (pivot, hint) with hint 1 = increasingHint, 2 = decreasingHint, 0 = unknownHint."""
    swaps = [0]

    def order2(x, y):
        if data.less(y, x):
            swaps[0] += 1
            return y, x
        return x, y

    def median(x, y, z):
        x, y = order2(x, y)
        y, z = order2(y, z)
        x, y = order2(x, y)
        return y

    n = b - a
    i, j, k = a + n // 4 * 1, a + n // 4 * 2, a + n // 4 * 3
    if n >= 8:
        if n >= 50:
            i = median(i - 1, i, i + 1)
            j = median(j - 1, j, j + 1)
            k = median(k - 1, k, k + 1)
        j = median(i, j, k)
    return j, 1 if swaps[0] == 0 else 2 if swaps[0] == 12 else 0


def go_partial_insertion_sort(data, a, b):
    i = a + 1
    for _ in range(5):
        while i < b and not data.less(i, i - 1):
            i += 1
        if i == b:
            return True
        if b - a < 50:
            return False
        data.swap(i, i - 1)
        if i - a >= 2:
            for j in range(i - 1, 0, -1):
                if not data.less(j, j - 1):
                    break
                data.swap(j, j - 1)
        if b - i >= 2:
            for j in range(i + 1, b):
                if not data.less(j, j - 1):
                    break
                data.swap(j, j - 1)
    return False


def go_top_frame(pairs):
    """pdqsort_func's first frame for n > 12: returns (finished, hint, data).  finished: the frame returned
    from partialInsertionSort with the array sorted; otherwise the general pdqsort goes on from `data`."""
    data = Data(pairs)
    n = len(pairs)
    _, hint = go_choose_pivot(data, 0, n)
    if hint == 1 and go_partial_insertion_sort(data, 0, n):
        return True, hint, data.d
    return False, hint, data.d


def closed_applies(pairs, pos):
    """The kernel's test before it takes the closed form (anything else falls to the general sort_claims)."""
    n = len(pairs)
    if pos < 0 or n < 50 or pos + 1 >= n or not pairs[pos][0] > pairs[pos + 1][0]:
        return False
    return go_choose_pivot(Data(pairs), 0, n)[1] == 1


def closed_form(pairs, pos):
    """(array, tlo, thi) as the kernel computes them: t by ballots over 64-entry chunks that stop at the first
    chunk holding an entry not below the claim's key, then the shift over (pos, pos+t] in chunks, low chunk
    first, each chunk read whole before it is written, then the claim's entry at pos + t."""
    d = list(pairs)
    n = len(d)
    claim = d[pos]
    t = 0
    for base in range(pos + 1, n, WAVE):
        below = [q < n and d[q][0] < claim[0] for q in range(base, base + WAVE)]
        t += sum(below)
        if not all(below):
            break
    for lo in range(pos + 1, pos + t + 1, WAVE):
        hi = min(lo + WAVE, pos + t + 1)
        chunk = [d[j] for j in range(lo, hi)]
        for j, e in zip(range(lo, hi), chunk):
            d[j - 1] = e
    d[pos + t] = claim
    return d, pos, pos + t


def crossings(keys):
    """Every array a single count crossing leaves: keys non-decreasing, one entry of a tie lifted by one."""
    for pos in range(len(keys) - 1):
        if keys[pos] == keys[pos + 1]:
            k = list(keys)
            k[pos] += 1
            yield pos, [(x, i) for i, x in enumerate(k)]


def check(pairs, pos, tally):
    n = len(pairs)
    finished, hint, want = go_top_frame(pairs)
    take = closed_applies(pairs, pos)
    assert take == (n >= 50 and hint == 1), (n, pos, hint)
    if n >= 50:
        tally[0] += 1
        tally[1] += take
    if not take:
        # the model's own result is the reference: below 50 entries the frame moves nothing and hands the
        # array to the general sort
        if n < 50:
            assert not finished and want == list(pairs)
        return
    assert finished, (n, pos)
    got, tlo, thi = closed_form(pairs, pos)
    assert got == want, (n, pos)
    moved = [i for i in range(n) if pairs[i] != want[i]]
    assert moved and tlo == moved[0] and thi == moved[-1], (n, pos, tlo, thi)
    assert all(got[i][0] <= got[i + 1][0] for i in range(n - 1))


def test_closed_form_matches_go_top_frame_on_tied_arrays():
    rng = random.Random(9)
    tally = [0, 0]
    cases = 0
    for n in range(13, 201):
        for width in (1, 3, 12):  # heavy ties down to a handful per count
            keys = sorted(rng.randint(1, 1 + max(1, n // width // 4)) for _ in range(n))
            for pos, pairs in crossings(keys):
                check(pairs, pos, tally)
                cases += 1
    assert cases > 15000
    print("cases %d, n >= 50: %d of which closed form %d" % (cases, tally[0], tally[1]))
    assert tally[1] >= 0.8 * tally[0], "the closed form must carry at least 80 %% of the n >= 50 cases: %s" % tally


def test_edges_of_the_crossing_position_and_the_tie_block():
    tally = [0, 0]
    for n in (13, 49, 50, 51, 64, 65, 66, 122, 129, 130, 131, 193, 194, 200):
        shapes = {
            "one tie block": [5] * n,  # pos = 0 .. n-2, blocks past 64 and 128 entries reaching the end
            "block at the end": list(range(n // 3)) + [n] * (n - n // 3),
            "block at the start": [2] * (n - n // 4) + list(range(3, 3 + n // 4)),
            "pairs": [i // 2 for i in range(n)],
        }
        for name, keys in shapes.items():
            assert keys == sorted(keys) and len(keys) == n
            seen = set()
            for pos, pairs in crossings(keys):
                check(pairs, pos, tally)
                seen.add(pos)
            if name == "one tie block":
                assert seen == set(range(n - 1))  # pos = 0 and pos = n - 2 among them
    # blocks longer than one and two waves were shifted through the closed form
    pairs = [(5, i) for i in range(200)]
    pairs[0] = (6, 0)
    assert closed_applies(pairs, 0)
    got, tlo, thi = closed_form(pairs, 0)
    assert (tlo, thi) == (0, 199) and got[199] == (6, 0) and got[:199] == [(5, i) for i in range(1, 200)]
    pairs = [(5, i) for i in range(200)]
    pairs[198] = (6, 198)
    assert closed_applies(pairs, 198)
    got, tlo, thi = closed_form(pairs, 198)
    assert (tlo, thi) == (198, 199) and got[198] == (5, 199) and got[199] == (6, 198)
    assert tally[1] >= 0.8 * tally[0], tally


def test_the_precondition_is_required():
    """An array with no descent at pos, or with an appended claim (count 1 behind greater counts), is not the
    closed form's: the kernel's test refuses both."""
    pairs = [(i // 3, i) for i in range(90)]
    assert not closed_applies(pairs, 10)
    assert not closed_applies(pairs, -1)
    assert not closed_applies(pairs, 89)
