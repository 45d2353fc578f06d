// ks_sort_regs.h — the general claim re-sort (partialInsertionSort, then Go's pdqsort_func: ks_gosort.h) on a copy of
// up to 128 (key, claim id) entries held across one wave's lanes: lane l holds positions l and 64 + l.  A key at a
// uniform position is a readlane, a count is a ballot, an exchange is a select on the lane id, a shift or a reversal
// is a lane permutation: nothing goes through memory between the load and the store.
//
// The algorithm is written once, over a wave-ops policy W:
//   W::Vec                  one 32-bit value per lane
//   W::each(f)              f(l) for every lane l (a per-lane instruction sequence: it reads and writes lane l only)
//   W::at(v, l), get(v, l)  lane l's element of v (inside each / ballot / gather / scatter functors)
//   W::rdl(v, l)            the element of the uniform lane l
//   W::ballot(p)            bit l = p(l)
//   W::gather(v, src)       r[l] = v[src(l)]  (a pull: ds_bpermute)
//   W::scatter(v, dst)      r[dst(l)] = v[l], dst a bijection of the 64 lanes  (a push: ds_permute)
// The kernels' policy maps these to the wave builtins (ks_solve.hip); SortRegsHostOps below emulates the 64 lanes with
// plain arrays, every operation applied to all lanes before the next, which is what lets the replay be compared with
// GoSortExact on the host (tests/test_sort_regs_model.py, scripts/sort_regs_host_main.cpp).  Host-only-safe.
//
// The copy may be abandoned at any point (`bail`): the arrays it was loaded from are written only by store().  Every
// loop is bounded by a constant or by n, so a mistake shows as a bail-out or a wrong order, not as a hang.
#pragma once
#include <stdint.h>

#include "ks_gosort.h"

namespace ks {

constexpr int kSortRegsMax = 128;  // entries the copy holds (two per lane)

// choosePivot_func's medians (zsortfunc.go) on the keys of its samples: k<3 * g + t> is the key at
// (a + l/4 * (g + 1)) + t - 1; below 50 entries only t = 1 is read.  Same pivot and hint as GoSortT::choosePivot.
// (Nine scalars, not an array: nothing here may become a stack object in the kernels.)
// ClaimSort::w_choose_pivot_at (ks_solve.hip) holds the same medians for the LDS form: a change here is a change there.
KS_HD int choose_pivot_medians(int a, int b, int& hint, int k0, int k1, int k2, int k3, int k4, int k5, int k6, int k7,
                               int k8) {
  const int l = b - a;
  int i = a + l / 4, j = a + l / 4 * 2, k = a + l / 4 * 3, swaps = 0;
  if (l >= 8) {
    auto median = [&](int ia, int ka, int ib, int kb, int ic, int kc, int& km) {
      if (kb < ka) { swaps++; int t0 = ia; ia = ib; ib = t0; t0 = ka; ka = kb; kb = t0; }
      if (kc < kb) { swaps++; int t0 = ib; ib = ic; ic = t0; t0 = kb; kb = kc; kc = t0; }
      if (kb < ka) { swaps++; int t0 = ia; ia = ib; ib = t0; t0 = ka; ka = kb; kb = t0; }
      km = kb;
      return ib;
    };
    int ki = k1, kj = k4, kq = k7;
    if (l >= 50) {
      i = median(i - 1, k0, i, k1, i + 1, k2, ki);
      j = median(j - 1, k3, j, k4, j + 1, k5, kj);
      k = median(k - 1, k6, k, k7, k + 1, k8, kq);
    }
    int km = 0;
    j = median(i, ki, j, kj, k, kq, km);
  }
  hint = swaps == 0 ? 1 : (swaps == 12 ? 2 : 0);
  return j;
}

// TWO: positions 64 .. 127 are held as well (false: n <= 64, one pair of registers per lane)
template <class W, bool TWO>
struct SortRegsT {
  using Vec = typename W::Vec;
  Vec k0, v0, k1, v1;  // keys and claim ids of positions l (k0, v0) and 64 + l (k1, v1)
  int n = 0;
  int bail = 0;    // an invariant failed: the copy is abandoned
  int breaks = 0;  // breakPatterns calls (the tests prove their regime with it)
  int heaps = 0;   // heapSort calls (the depth limit)

  static KS_HD int popc(uint64_t m) { return __builtin_popcountll(m); }
  static KS_HD int lowbit(uint64_t m) { return __builtin_ctzll(m); }         // m != 0
  static KS_HD int highbit(uint64_t m) { return 63 - __builtin_clzll(m); }   // m != 0

  // positions >= n hold a sentinel no predicate selects (each is also masked by its range)
  template <class KF, class VF>
  KS_HD void load(int n_, KF keyOf, VF valOf) {
    n = n_;
    W::each([&](int l) {
      W::at(k0, l) = l < n ? keyOf(l) : INT32_MAX;
      W::at(v0, l) = l < n ? valOf(l) : -1;
      if (TWO) {
        W::at(k1, l) = 64 + l < n ? keyOf(64 + l) : INT32_MAX;
        W::at(v1, l) = 64 + l < n ? valOf(64 + l) : -1;
      }
    });
  }
  template <class PF>
  KS_HD void store(PF put) const {
    W::each([&](int l) {
      if (l < n) put(l, W::get(k0, l), W::get(v0, l));
      if (TWO && 64 + l < n) put(64 + l, W::get(k1, l), W::get(v1, l));
    });
  }

  KS_HD int keyAt(int p) const {
    const int lo = W::rdl(k0, p & 63);
    if (!TWO) return lo;
    const int hi = W::rdl(k1, p & 63);
    return p < 64 ? lo : hi;
  }
  KS_HD int valAt(int p) const {
    const int lo = W::rdl(v0, p & 63);
    if (!TWO) return lo;
    const int hi = W::rdl(v1, p & 63);
    return p < 64 ? lo : hi;
  }
  KS_HD void setKey(int p, int k) {
    W::each([&](int l) {
      W::at(k0, l) = l == p ? k : W::get(k0, l);
      if (TWO) W::at(k1, l) = 64 + l == p ? k : W::get(k1, l);
    });
  }
  KS_HD void setVal(int p, int v) {
    W::each([&](int l) {
      W::at(v0, l) = l == p ? v : W::get(v0, l);
      if (TWO) W::at(v1, l) = 64 + l == p ? v : W::get(v1, l);
    });
  }
  // exchange of two uniform positions
  KS_HD void swap(int i, int j) {
    const int ki = keyAt(i), vi = valAt(i), kj = keyAt(j), vj = valAt(j);
    W::each([&, i, j, ki, vi, kj, vj](int l) {
      W::at(k0, l) = l == i ? kj : l == j ? ki : W::get(k0, l);
      W::at(v0, l) = l == i ? vj : l == j ? vi : W::get(v0, l);
      if (TWO) {
        W::at(k1, l) = 64 + l == i ? kj : 64 + l == j ? ki : W::get(k1, l);
        W::at(v1, l) = 64 + l == i ? vj : 64 + l == j ? vi : W::get(v1, l);
      }
    });
  }
  // bit l of m0 / m1 = pred(position, key) at l / 64 + l
  template <class F>
  KS_HD void masks(F pred, uint64_t& m0, uint64_t& m1) const {
    m0 = W::ballot([&](int l) { return pred(l, W::get(k0, l)); });
    m1 = 0;
    if (TWO) m1 = W::ballot([&](int l) { return pred(64 + l, W::get(k1, l)); });
  }
  // new[p] = old[src(p)] for every position p (src(p) = p: unchanged)
  template <class F>
  KS_HD void pull(F src) {
    const auto s0 = [&](int l) { return src(l) & 63; };
    const Vec a0 = W::gather(k0, s0), b0 = W::gather(v0, s0);
    if (!TWO) {
      k0 = a0;
      v0 = b0;
      return;
    }
    const auto s1 = [&](int l) { return src(64 + l) & 63; };
    const Vec a1 = W::gather(k1, s0), b1 = W::gather(v1, s0);
    const Vec c0 = W::gather(k0, s1), d0 = W::gather(v0, s1), c1 = W::gather(k1, s1), d1 = W::gather(v1, s1);
    W::each([&](int l) {
      const bool lo0 = src(l) < 64, lo1 = src(64 + l) < 64;
      W::at(k0, l) = lo0 ? W::get(a0, l) : W::get(a1, l);
      W::at(v0, l) = lo0 ? W::get(b0, l) : W::get(b1, l);
      W::at(k1, l) = lo1 ? W::get(c0, l) : W::get(c1, l);
      W::at(v1, l) = lo1 ? W::get(d0, l) : W::get(d1, l);
    });
  }

  // ClaimSort::pis_move: the entry at `from` to `to`, the ones between one place towards `from`
  KS_HD void move(int from, int to) {
    if (from == to) return;
    if (to < from) pull([=](int p) { return p == to ? from : (p > to && p <= from) ? p - 1 : p; });
    else pull([=](int p) { return p == to ? from : (p >= from && p < to) ? p + 1 : p; });
  }
  KS_HD void reverse(int a, int b) {
    pull([=](int p) { return p >= a && p < b ? a + b - 1 - p : p; });
  }
  // first i in [from, b) with key[i] < key[i-1], or b (from >= 1)
  KS_HD int descent(int from, int b) const {
    const auto prev = [](int l) { return (l + 63) & 63; };
    const Vec p0 = W::gather(k0, prev);  // lane 0 holds key[63]: position 64's left neighbour
    uint64_t m0 = W::ballot([&](int l) { return l >= from && l < b && W::get(k0, l) < W::get(p0, l); }), m1 = 0;
    if (TWO) {
      const Vec p1 = W::gather(k1, prev);
      m1 = W::ballot([&](int l) {
        return 64 + l >= from && 64 + l < b && W::get(k1, l) < (l == 0 ? W::get(p0, l) : W::get(p1, l));
      });
    }
    return m0 ? lowbit(m0) : m1 ? 64 + lowbit(m1) : b;
  }
  // ClaimSort::pis_wave (partialInsertionSort_func of Go 1.21)
  KS_HD bool pis(int a, int b, int& tlo, int& thi) {
    int i = a + 1;
    for (int step = 0; step < 5; step++) {
      i = descent(i, b);
      if (i == b) return true;
      if (b - a < 50) return false;
      const int x = keyAt(i), y = keyAt(i - 1);  // after the swap: x at i-1, y at i
      int p = i - 1;  // x passes the entries q < i-1 with x < key[q] (down to index 1, not to a)
      if (i - a >= 2) {
        uint64_t m0, m1;
        masks([=](int q, int k) { return q < i - 1 && !(x < k); }, m0, m1);
        p = m1 ? 64 + highbit(m1) + 1 : m0 ? highbit(m0) + 1 : 0;
      }
      int r = i;  // y passes the entries q > i with key[q] < y
      if (i + 1 < b) {
        uint64_t m0, m1;
        masks([=](int q, int k) { return q > i && q < b && !(k < y); }, m0, m1);
        r = m0 ? lowbit(m0) - 1 : m1 ? 64 + lowbit(m1) - 1 : b - 1;
      }
      move(i, p);  // x (at i before the swap) to p; y moves from i-1 to i with the shifted run
      move(i, r);  // y to r
      tlo = p < tlo ? p : tlo;
      thi = r > thi ? r : thi;
    }
    return false;
  }
  KS_HD int choose(int a, int b, int& hint) const {
    const int l = b - a, i = a + l / 4, j = a + l / 4 * 2, k = a + l / 4 * 3;
    int s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, s7 = 0, s8 = 0;
    if (l >= 8) {
      s1 = keyAt(i);
      s4 = keyAt(j);
      s7 = keyAt(k);
      if (l >= 50) {
        s0 = keyAt(i - 1); s2 = keyAt(i + 1);
        s3 = keyAt(j - 1); s5 = keyAt(j + 1);
        s6 = keyAt(k - 1); s8 = keyAt(k + 1);
      }
    }
    return choose_pivot_medians(a, b, hint, s0, s1, s2, s3, s4, s5, s6, s7, s8);
  }
  // entries of [a, b) whose key is below `pk` (below_or_eq: at most `pk`)
  KS_HD int count(int a, int b, int pk, bool below_or_eq) const {
    uint64_t m0, m1;
    masks([=](int p, int k) { return p >= a && p < b && (below_or_eq ? k <= pk : k < pk); }, m0, m1);
    return popc(m0) + popc(m1);
  }
  // ClaimSort::w_hoare: the k-th wrong-side entry from the bottom of [l0, m) with the k-th from the top of [m, r1)
  KS_HD int hoare(int l0, int m, int r1, int pk, bool eq) {
    uint64_t L0, L1, R0, R1;
    masks([=](int p, int k) { return p >= l0 && p < m && (eq ? k > pk : k >= pk); }, L0, L1);
    masks([=](int p, int k) { return p >= m && p < r1 && (eq ? k <= pk : k < pk); }, R0, R1);
    const int nL = popc(L0) + popc(L1);
    if (nL != popc(R0) + popc(R1)) {
      bail = 1;
      return 0;
    }
    for (int t = 0; t < nL; t++) {
      int i, j;
      if (L0) { i = lowbit(L0); L0 &= L0 - 1; }
      else { i = 64 + lowbit(L1); L1 &= L1 - 1; }
      if (R1) { const int h = highbit(R1); j = 64 + h; R1 &= ~(1ull << h); }
      else { const int h = highbit(R0); j = h; R0 &= ~(1ull << h); }
      swap(i, j);
    }
    return nL;
  }
  KS_HD int partition(int a, int b, int pivot, bool& already) {
    swap(a, pivot);
    const int pk = keyAt(a);
    const int j = a + count(a + 1, b, pk, false);
    already = hoare(a + 1, j + 1, b, pk, false) == 0;
    swap(j, a);
    return j;
  }
  KS_HD int partition_equal(int a, int b, int pivot) {
    swap(a, pivot);
    const int pk = keyAt(a);
    const int m = a + 1 + count(a + 1, b, pk, true);
    hoare(a + 1, m, b, pk, true);
    return m;
  }
  // insertionSort_func on [a, b), b - a <= 12: a stable sort, so the stable-rank permutation (ClaimSort::w_leaf).
  // A range inside one half is ranked per lane and pushed to its rank; one across position 64 is ranked entry by
  // entry on the old values.
  KS_HD void leaf_half(Vec& kh, Vec& vh, int a, int b) {  // lane positions of one half
    Vec rank;
    W::each([&](int l) { W::at(rank, l) = 0; });
    for (int j = a; j < b; j++) {
      const int kj = W::rdl(kh, j);
      W::each([&](int l) {
        const int mk = W::get(kh, l);
        W::at(rank, l) += kj < mk || (kj == mk && j < l) ? 1 : 0;
      });
    }
    const auto dst = [&](int l) { return l >= a && l < b ? a + W::get(rank, l) : l; };  // rank < b - a: a bijection
    kh = W::scatter(kh, dst);
    vh = W::scatter(vh, dst);
  }
  KS_HD void leaf(int a, int b) {
    if (b - a < 2) return;
    if (!TWO || b <= 64) return leaf_half(k0, v0, a, b);
    if (a >= 64) return leaf_half(k1, v1, a - 64, b - 64);
    const SortRegsT old = *this;
    for (int pj = a; pj < b; pj++) {
      const int kj = old.keyAt(pj), vj = old.valAt(pj);
      uint64_t m0, m1;
      old.masks([=](int p, int k) { return p >= a && p < b && (k < kj || (k == kj && p < pj)); }, m0, m1);
      const int d = a + popc(m0) + popc(m1);
      setKey(d, kj);
      setVal(d, vj);
    }
  }
  // breakPatterns and heapSort are rare (an unbalanced partition, the depth limit): GoSortT itself runs them, its
  // arrays being these proxies -- a read is keyAt / valAt, a write a select on the lane.
  struct Proxy {
    SortRegsT* s;
    bool val;
    struct Ref {
      SortRegsT* s;
      bool val;
      int p;
      KS_HD operator int32_t() const { return val ? s->valAt(p) : s->keyAt(p); }
      KS_HD Ref& operator=(int32_t x) {
        if (val) s->setVal(p, x);
        else s->setKey(p, x);
        return *this;
      }
      KS_HD Ref& operator=(const Ref& o) { return *this = (int32_t)o; }
    };
    KS_HD Ref operator[](int p) const { return Ref{s, val, p}; }
  };

  // heapSort_func on [a, b) through the proxies (scripts/sort_regs_host_main.cpp also calls it directly)
  KS_HD void heap(int a, int b) {
    GoSortT<Proxy> g{Proxy{this, false}, Proxy{this, true}};
    g.heapSort(a, b);
    heaps++;
  }

  // GoSortExactT::run as ClaimSort::w_pdqsort runs it: the frames live one per lane (lane k = stack slot k)
  KS_HD void pdq(int resumePivot) {
    Vec fa, fb, fl, ff;  // a, b, limit, flags (wb | wp << 1)
    const int maxsp = 2 * GoSortT<int32_t*>::bitsLen((uint32_t)n) + 2;  // <= 18 lanes
    int budget = 4 * n + 8;  // frames (<= 2n + 1, a partition each pair) plus partitionEquals (each drops an entry)
    const int lim0 = GoSortT<int32_t*>::bitsLen((uint32_t)n);
    W::each([&](int l) {
      W::at(fa, l) = 0;
      W::at(fb, l) = n;
      W::at(fl, l) = lim0;
      W::at(ff, l) = 3;
    });
    int sp = 1;
    bool resume = resumePivot >= 0;
    int dummy_lo = 0, dummy_hi = 0;
    while (sp > 0) {
      sp--;
      int a = W::rdl(fa, sp), b = W::rdl(fb, sp), limit = W::rdl(fl, sp);
      const int flags = W::rdl(ff, sp);
      bool wasBalanced = flags & 1, wasPartitioned = (flags >> 1) & 1;
      for (;;) {
        if (--budget < 0) {
          bail = 1;
          return;
        }
        const int length = b - a;
        int pivot;
        if (resume) {
          resume = false;
          pivot = resumePivot;
        } else {
          if (length <= 12) {
            leaf(a, b);
            break;
          }
          if (limit == 0) {
            heap(a, b);
            break;
          }
          if (!wasBalanced) {
            GoSortT<Proxy> g{Proxy{this, false}, Proxy{this, true}};
            g.breakPatterns(a, b);
            breaks++;
            limit--;
          }
          int hint = 0;
          pivot = choose(a, b, hint);
          if (hint == 2) {
            reverse(a, b);
            pivot = (b - 1) - (pivot - a);
            hint = 1;
          }
          if (wasBalanced && wasPartitioned && hint == 1 && pis(a, b, dummy_lo, dummy_hi)) break;
        }
        if (a > 0 && !(keyAt(a - 1) < keyAt(pivot))) {
          a = partition_equal(a, b, pivot);
          if (bail) return;
          continue;
        }
        bool already = false;
        const int mid = partition(a, b, pivot, already);
        if (bail) return;
        wasPartitioned = already;
        const int leftLen = mid - a, rightLen = b - mid, thr = length / 8;
        if (sp + 2 > maxsp) {
          bail = 1;
          return;
        }
        int c0a, c0b, c1a, c1b;
        if (leftLen < rightLen) {
          wasBalanced = leftLen >= thr;
          c0a = mid + 1; c0b = b; c1a = a; c1b = mid;  // continuation, then the recursive call
        } else {
          wasBalanced = rightLen >= thr;
          c0a = a; c0b = mid; c1a = mid + 1; c1b = b;
        }
        const int f0 = (int)wasBalanced | ((int)wasPartitioned << 1);
        // (the scalars by value: selects among references captured by a closure become selects of addresses,
        // and the closure a stack object)
        W::each([&, c0a, c0b, c1a, c1b, limit, f0, sp](int l) {
          const bool m0 = l == sp, m1 = l == sp + 1;
          W::at(fa, l) = m0 ? c0a : m1 ? c1a : W::get(fa, l);
          W::at(fb, l) = m0 ? c0b : m1 ? c1b : W::get(fb, l);
          W::at(fl, l) = m0 || m1 ? limit : W::get(fl, l);
          W::at(ff, l) = m0 ? f0 : m1 ? 3 : W::get(ff, l);
        });
        sp += 2;
        break;
      }
    }
  }
  // claim_sort_general on the copy: partialInsertionSort when choosePivot gave the increasing hint (pivot >= 0),
  // else or after it the exact pdqsort.  Returns claim_sort_general's word with kSortRegsDone set, or 0 after a
  // bail-out (nothing to store).
  KS_HD uint32_t general(int pivot) {
    int tlo = n, thi = -1;
    bool done = false;
    if (pivot >= 0) done = pis(0, n, tlo, thi);
    if (!done) {
      pdq(pivot);
      tlo = 0;
      thi = n - 1;
    }
    if (bail) return 0;
    return (uint32_t)tlo | (uint32_t)(thi + 1) << 15 | (uint32_t)done << 30 | 1u << 31;
  }
};
constexpr uint32_t kSortRegsDone = 1u << 31;  // claim_sort_general's word: the re-sort finished on the register copy

// 64 lanes as plain arrays, each operation applied to all lanes before the next
struct SortRegsHostOps {
  struct Vec { int32_t x[64]; };
  template <class F> static void each(F f) { for (int l = 0; l < 64; l++) f(l); }
  static int32_t& at(Vec& v, int l) { return v.x[l]; }
  static int32_t get(const Vec& v, int l) { return v.x[l]; }
  static int32_t rdl(const Vec& v, int l) { return v.x[l & 63]; }
  template <class F> static uint64_t ballot(F p) {
    uint64_t m = 0;
    for (int l = 0; l < 64; l++) m |= p(l) ? 1ull << l : 0ull;
    return m;
  }
  template <class F> static Vec gather(const Vec& v, F src) {
    Vec r;
    for (int l = 0; l < 64; l++) r.x[l] = v.x[src(l) & 63];
    return r;
  }
  template <class F> static Vec scatter(const Vec& v, F dst) {
    Vec r;
    for (int l = 0; l < 64; l++) r.x[l] = INT32_MIN;  // (a lane no one pushes to: not a bijection, and it shows)
    for (int l = 0; l < 64; l++) r.x[dst(l) & 63] = v.x[l];
    return r;
  }
};

// The lane model of claim_sort_general on host arrays: choosePivot's hint as Solver::sort_claims takes it, then the
// register path (two: 128 entries, else 64), and Go's pdqsort_func on the untouched arrays when it did not finish.
// Returns how (0: partialInsertionSort finished it, 1: the exact sort ran); *path = 1 (registers), 2 (an invariant
// failed: a bail-out) or 3 (more entries than the copy holds), plus the breakPatterns calls << 8 and the heapSort
// calls << 20.
inline int sort_regs_model(int n, int32_t* keys, int32_t* order, bool two, int* path) {
  int pivot = -1;
  if (n > 12) {
    GoSort g{keys, order};
    int hint = 0;
    const int pv = g.choosePivot(0, n, hint);
    if (hint == 1) pivot = pv;
  }
  uint32_t word = 0;
  int breaks = 0, heaps = 0;
  const bool fits = n <= (two ? kSortRegsMax : 64);
  if (fits) {
    const auto run = [&](auto& rs) {
      rs.load(n, [&](int p) { return keys[p]; }, [&](int p) { return order[p]; });
      word = rs.general(pivot);
      breaks = rs.breaks;
      heaps = rs.heaps;
      if (word) rs.store([&](int p, int k, int v) { keys[p] = k; order[p] = v; });
    };
    if (two) {
      SortRegsT<SortRegsHostOps, true> rs;
      run(rs);
    } else {
      SortRegsT<SortRegsHostOps, false> rs;
      run(rs);
    }
  }
  if (path) *path = (word ? 1 : fits ? 2 : 3) | breaks << 8 | heaps << 20;
  if (word) return word >> 30 & 1 ? 0 : 1;
  GoSortExact g{GoSort{keys, order}};
  g.run(n);
  return 1;
}

}  // namespace ks
