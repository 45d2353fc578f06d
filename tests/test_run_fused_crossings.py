"""The LEAN Solve's deferred move of a run's claim (KS_RUN_FUSE), on the model of
test_sort_single_descent.py.

A run of identical pods stays on its NodeClaim across re-sorts.  Each closed-form crossing lifts the claim over
the block of entries below its count and moves nothing else, so the kernel leaves the position arrays as they are
while the run advances and carries (pos0, p, K): the array the next add() would sort has the claim's entry taken
from pos0 and put at p with count K, the entries between one place to the left.  Checked here, payloads included:

* k successive single crossings (each the Go top frame's own result) equal that one composed shift;
* choosePivot read through the index map (i in [pos0, p) reads i + 1, p reads K) returns the pivot and hint of
  choosePivot on the materialised array, at every crossing -- the descent next to and on each of the nine samples;
* below 50 entries and on any other hint the closed form is not taken (the kernel materialises and runs the
  general re-sort)."""
import random

from test_sort_single_descent import Data, closed_applies, closed_form, go_choose_pivot, go_top_frame

WAVE = 64


class Moved(Data):
    """The physical array read through the deferred move's index map (ClaimSort::w_choose_pivot_moved)."""

    def __init__(self, phys, pos0, p, K):
        self.phys, self.pos0, self.p, self.K = phys, pos0, p, K

    def key(self, i):
        if i == self.p:
            return self.K
        return self.phys[i + 1 if self.pos0 <= i < self.p else i][0]

    def less(self, i, j):
        return self.key(i) < self.key(j)

    def swap(self, i, j):
        raise AssertionError("choosePivot only reads")


def materialise(phys, pos0, p, K):
    """Solver::run_materialise: (pos0, p] one place left (pis_move), the claim's entry at p with count K."""
    d = list(phys)
    claim = d[pos0][1]
    d[pos0:p] = phys[pos0 + 1:p + 1]
    d[p] = (K, claim)
    return d


def count_below(phys, p, K):
    """Solver::run_count_below: ballots over 64-entry chunks, four per round, up to the first entry not below K."""
    n, t = len(phys), 0
    for base in range(p + 1, n, WAVE):
        below = [q < n and phys[q][0] < K for q in range(base, base + WAVE)]
        t += sum(below)
        if not all(below):
            break
    return t


def run(keys, pos0, tally):
    """One run on the claim at pos0 of a sorted array: segment after segment lifts its count to one above the
    next position's; the step-by-step array `a` goes through every crossing for real, the fused state never
    touches `phys`.  Returns the crossings taken in closed form."""
    n = len(keys)
    phys = [(x, i) for i, x in enumerate(keys)]
    a, pos = list(phys), pos0  # step by step
    p, K = pos0, keys[pos0]    # fused
    crossed = 0
    while p + 1 < n:
        K = phys[p + 1][0] + 1  # the pod that lifts the count past the next position's
        a[pos] = (K, a[pos][1])
        assert a == materialise(phys, pos0, p, K), (n, pos0, p)
        want = go_choose_pivot(Data(a), 0, n)
        assert go_choose_pivot(Moved(phys, pos0, p, K), 0, n) == want, (n, pos0, p)
        take = n >= 50 and want[1] == 1
        assert take == closed_applies(a, pos)
        tally[0] += 1
        tally[1] += take
        if not take:
            break  # the kernel materialises (checked above) and runs the general re-sort
        finished, _, after = go_top_frame(a)
        assert finished
        a, tlo, thi = closed_form(a, pos)
        assert a == after and tlo == pos
        t = count_below(phys, p, K)
        assert thi == pos + t
        pos = thi
        p += t
        crossed += 1
    assert a == materialise(phys, pos0, p, K)
    return crossed


def test_composed_shift_on_random_tied_arrays():
    rng = random.Random(10)
    tally, multi = [0, 0], 0
    for n in list(range(13, 131)) + [192, 193, 200]:
        for width in (1, 3, 12):
            keys = sorted(rng.randint(1, 1 + max(1, n // width // 4)) for _ in range(n))
            for pos0 in rng.sample(range(n - 1), min(n - 1, 12)):
                multi += run(keys, pos0, tally) >= 2
    print("crossings %d, closed form %d, runs over two or more tie blocks %d" % (tally[0], tally[1], multi))
    assert multi > 500


def test_every_start_at_the_closed_form_s_size_threshold():
    """n = 49 never takes it, 50 and 51 do: every start position, so the descent stands on and next to each of
    choosePivot's nine samples, inside and outside the shifted range."""
    for n in (49, 50, 51, 64, 65, 129):
        shapes = [[5] * n, [i // 2 for i in range(n)], [i // 7 for i in range(n)],
                  list(range(n // 3)) + [n] * (n - n // 3)]
        for keys in shapes:
            tally = [0, 0]
            for pos0 in range(n - 1):
                run(keys, pos0, tally)
            if n < 50:
                assert tally[1] == 0
            else:
                assert tally[1] > 0
    # the samples themselves: a run that starts before the first sample and crosses blocks past the last one
    n = 100
    keys = [i // 3 for i in range(n)]
    samples = {q * (n // 4) + d for q in (1, 2, 3) for d in (-1, 0, 1)}
    at = set()
    phys = [(x, i) for i, x in enumerate(keys)]
    p, pos0 = 2, 2
    while p + 1 < n:
        K = phys[p + 1][0] + 1
        a = materialise(phys, pos0, p, K)
        assert go_choose_pivot(Moved(phys, pos0, p, K), 0, n) == go_choose_pivot(Data(a), 0, n)
        at |= {p + d for d in (-1, 0, 1)} & samples
        p += count_below(phys, p, K)
    assert at == samples
