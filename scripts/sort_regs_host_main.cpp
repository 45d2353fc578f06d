// Stand-alone driver of the register-copy claim re-sort's lane model (csrc/ks_sort_regs.h with SortRegsHostOps)
// against Go's pdqsort_func (csrc/ks_gosort.h) for AddressSanitizer + UndefinedBehaviorSanitizer;
// scripts/sort_regs_asan.sh builds and runs it.  The sweep is tests/test_sort_regs_model.py's.  No HIP runtime, no
// device.  Exits non-zero on a differing result; a sanitizer report aborts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../karpenter-sigs_amd/csrc/ks_sort_regs.h"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 11);
}

static long cases = 0, viaRegs = 0, bails = 0, breaks = 0, heaps = 0, heapCases = 0;

// the model in both widths against Go; false on a difference
static bool check(const std::vector<int32_t>& keys, const char* what) {
  const int n = (int)keys.size();
  std::vector<int32_t> order(n);
  for (int i = 0; i < n; i++) order[i] = i;
  for (int i = n - 1; i > 0; i--) std::swap(order[i], order[rnd() % (uint32_t)(i + 1)]);
  // exactly n entries each: a read or write past the end is the sanitizer's to see
  std::vector<int32_t> wk = keys, wo = order;
  ks::GoSortExact g{ks::GoSort{wk.data(), wo.data()}};
  g.run(n);
  for (int two = 0; two < 2; two++) {
    std::vector<int32_t> mk = keys, mo = order;
    int path = 0;
    ks::sort_regs_model(n, mk.data(), mo.data(), two != 0, &path);
    const bool regs = (path & 0xff) == 1;
    if (n <= (two ? ks::kSortRegsMax : 64) && !regs) {
      std::fprintf(stderr, "sort_regs_host: bail-out (%s, n %d, two %d)\n", what, n, two);
      return false;
    }
    if (n > (two ? ks::kSortRegsMax : 64) && regs) {
      std::fprintf(stderr, "sort_regs_host: no bail-out (%s, n %d, two %d)\n", what, n, two);
      return false;
    }
    if (mk != wk || mo != wo) {
      std::fprintf(stderr, "sort_regs_host: differs from Go (%s, n %d, two %d)\n", what, n, two);
      return false;
    }
    cases++;
    viaRegs += regs;
    bails += !regs;
    breaks += path >> 8 & 0xfff;
    heaps += path >> 20;
    if ((path & 0xff) == 2) {
      std::fprintf(stderr, "sort_regs_host: an invariant failed inside the copy (%s, n %d, two %d)\n", what, n, two);
      return false;
    }
  }
  return true;
}

// heapSort_func through the copy's proxies (SortRegsT::heap, what pdq calls at the depth limit) against GoSortT's on
// plain arrays, over ranges inside one half and across position 64.  No input of the sweep drives pdqsort's limit
// to 0 within 128 entries (main reports how many did), so the path is checked where it can be reached.
template <bool TWO>
static bool heap_check(int n, int a, int b, int vals) {
  std::vector<int32_t> k(n), o(n);
  for (int i = 0; i < n; i++) { k[i] = (int32_t)(rnd() % (uint32_t)vals); o[i] = i; }
  std::vector<int32_t> wk = k, wo = o;
  ks::GoSort g{wk.data(), wo.data()};
  g.heapSort(a, b);
  ks::SortRegsT<ks::SortRegsHostOps, TWO> rs;
  rs.load(n, [&](int p) { return k[p]; }, [&](int p) { return o[p]; });
  rs.heap(a, b);
  rs.store([&](int p, int kk, int vv) { k[p] = kk; o[p] = vv; });
  heapCases++;
  if (k != wk || o != wo || rs.heaps != 1) {
    std::fprintf(stderr, "sort_regs_host: heapSort differs from Go (n %d, [%d, %d), two %d)\n", n, a, b, (int)TWO);
    return false;
  }
  return true;
}

int main() {
  for (int vals : {2, 7, 1000})
    for (int rep = 0; rep < 3; rep++) {
      const int r64[][3] = {{64, 0, 64}, {64, 13, 40}, {20, 3, 17}, {1, 0, 1}, {2, 0, 2}};
      for (auto& c : r64)
        if (!heap_check<false>(c[0], c[1], c[2], vals) || !heap_check<true>(c[0], c[1], c[2], vals)) return 1;
      const int r128[][3] = {{128, 0, 128}, {128, 50, 90}, {128, 64, 128}, {100, 63, 66}, {65, 0, 65}};
      for (auto& c : r128)
        if (!heap_check<true>(c[0], c[1], c[2], vals)) return 1;
    }
  std::vector<int> lengths;
  for (int n = 0; n <= 128; n++) lengths.push_back(n);
  lengths.push_back(129);
  lengths.push_back(300);
  for (int n : lengths) {
    std::vector<int32_t> k(n);
    for (int i = 0; i < n; i++) k[i] = 5;
    if (!check(k, "equal")) return 1;
    for (int i = 0; i < n; i++) k[i] = i;
    if (!check(k, "increasing")) return 1;
    for (int i = 0; i < n; i++) k[i] = n - i;
    if (!check(k, "decreasing")) return 1;
    for (int seed = 0; seed < 3; seed++) {
      for (int i = 0; i < n; i++) k[i] = (int32_t)(rnd() % 2);
      if (!check(k, "random over 2")) return 1;
      for (int i = 0; i < n; i++) k[i] = (int32_t)(rnd() % (uint32_t)std::max(n / 2, 1));
      if (!check(k, "random over n/2")) return 1;
    }
    if (n >= 1) {  // one small key, then larger random ones: an unbalanced first partition
      k[0] = 0;
      for (int i = 1; i < n; i++) k[i] = 1 + (int32_t)(rnd() % 1000);
      if (!check(k, "unbalanced")) return 1;
    }
    // the workload's own shape: non-decreasing with ties, one entry lifted
    if (n < 2) continue;
    std::vector<int> poss = {0, n - 2};
    for (int q = 1; q <= 3; q++)
      for (int d = -1; d <= 1; d++) poss.push_back(q * (n / 4) + d);
    for (int w : {1, 3, 8})
      for (int lift : {1, w + 1})
        for (int pos : poss) {
          if (pos < 0 || pos >= n) continue;
          for (int i = 0; i < n; i++) k[i] = i / w;
          k[pos] += lift;
          if (!check(k, "lifted")) return 1;
        }
  }
  if (breaks == 0) {
    std::fprintf(stderr, "sort_regs_host: no case reached breakPatterns\n");
    return 1;
  }
  std::printf("sort_regs_host: %ld cases (%ld from registers, %ld beyond the copy, %ld breakPatterns, %ld heapSorts "
              "inside a sort), %ld direct heapSort cases, no reports\n", cases, viaRegs, bails, breaks, heaps, heapCases);
  return 0;
}
