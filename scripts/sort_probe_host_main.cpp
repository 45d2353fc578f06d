// Stand-alone driver of ks_claim_sort_probe's host side (csrc/ks_sort_probe.h: the argument check and Go's
// pdqsort_func with the regather) for AddressSanitizer + UndefinedBehaviorSanitizer; scripts/sort_probe_asan.sh
// builds and runs it.  No HIP runtime, no device.  Exits non-zero on a wrong result; a sanitizer report aborts.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../karpenter-sigs_amd/csrc/ks_sort_probe.h"

static uint64_t rng_state = 88172645463325252ull;
static uint32_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return (uint32_t)(rng_state >> 11);
}

static int fail(const char* what, int n, int shape) {
  std::fprintf(stderr, "sort_probe_host: %s (n %d, shape %d)\n", what, n, shape);
  return 1;
}

int main() {
  const int lengths[] = {0, 1, 2, 11, 12, 13, 24, 25, 49, 50, 51, 63, 64, 65, 127, 128, 129, 300, ks::kProbeMaxN};
  int cases = 0;
  for (int R = 3; R <= 4; R++)
    for (int n : lengths)
      for (int shape = 0; shape < 6; shape++) {
        // exactly n entries each: a read or write past the end is the sanitizer's to see
        std::vector<int32_t> keys(n), order(n), ctpl(n), ptpl(n);
        std::vector<int64_t> chead((size_t)n * R), phead((size_t)n * R);
        for (int i = 0; i < n; i++) {
          keys[i] = shape == 0 ? 5 : shape == 1 ? i : shape == 2 ? n - i : shape == 3 ? i / 3 + (i == n / 2)
                  : shape == 4 ? (int)(rnd() % 2) : (int)(rnd() % (uint32_t)std::max(n / 2, 1));
          order[i] = i;
          ctpl[i] = (i * 7 + 3) % 64;
          for (int r = 0; r < R; r++) chead[(size_t)i * R + r] = ((int64_t)i << 33) + 17 * r - 5;
        }
        for (int i = n - 1; i > 0; i--) std::swap(order[i], order[rnd() % (uint32_t)(i + 1)]);
        std::vector<std::pair<int32_t, int32_t>> before(n), after(n);
        for (int i = 0; i < n; i++) before[i] = {keys[i], order[i]};
        if (ks::sort_probe_check(0, -1, n, R, keys.data(), order.data(), ctpl.data(), chead.data(), ptpl.data(), phead.data()))
          return fail("valid arguments refused", n, shape);
        ks::sort_probe_host(n, R, keys.data(), order.data(), ctpl.data(), chead.data(), ptpl.data(), phead.data());
        if (!std::is_sorted(keys.begin(), keys.end())) return fail("not sorted", n, shape);
        for (int i = 0; i < n; i++) {
          after[i] = {keys[i], order[i]};
          if (ptpl[i] != ctpl[order[i]]) return fail("ptpl", n, shape);
          for (int r = 0; r < R; r++)
            if (phead[(size_t)i * R + r] != chead[(size_t)order[i] * R + r]) return fail("phead", n, shape);
        }
        std::sort(before.begin(), before.end());
        std::sort(after.begin(), after.end());
        if (before != after) return fail("pairs changed", n, shape);
        cases++;
      }
  // refused arguments: nothing is read or written
  std::vector<int32_t> k4 = {1, 2, 3, 4}, o4 = {0, 1, 2, 9}, t4(4), p4(4);
  std::vector<int64_t> h4(16), q4(16);
  if (!ks::sort_probe_check(0, -1, 4, 3, k4.data(), o4.data(), t4.data(), h4.data(), p4.data(), q4.data())) return fail("claim id 9 accepted", 4, 0);
  o4[3] = 3;
  if (!ks::sort_probe_check(1, 4, 4, 3, k4.data(), o4.data(), t4.data(), h4.data(), p4.data(), q4.data())) return fail("pos 4 accepted", 4, 0);
  if (!ks::sort_probe_check(0, -1, 4, 5, k4.data(), o4.data(), t4.data(), h4.data(), p4.data(), q4.data())) return fail("R 5 accepted", 4, 0);
  if (!ks::sort_probe_check(0, -1, ks::kProbeMaxN + 1, 3, k4.data(), o4.data(), t4.data(), h4.data(), p4.data(), q4.data())) return fail("n accepted", 4, 0);
  if (!ks::sort_probe_check(0, -1, 4, 3, nullptr, o4.data(), t4.data(), h4.data(), p4.data(), q4.data())) return fail("null accepted", 4, 0);
  std::printf("sort_probe_host: %d cases, no reports\n", cases);
  return 0;
}
