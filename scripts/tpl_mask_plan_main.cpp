// Stand-alone driver of the LEAN Solve's mask-table arithmetic (csrc/ks_tplmask.h: the words the kernel carves, the
// bytes make_plan counts, the test for keeping the table) for AddressSanitizer + UndefinedBehaviorSanitizer;
// scripts/tpl_mask_plan_asan.sh builds and runs it.  No HIP runtime, no device.  The kernel's carve and its row
// stores (try_templates' store_bits per 64-position chunk, then the template's flag word) are replayed on a heap
// buffer of exactly the planned size, so a store outside a row's words is a sanitizer report.  Exits non-zero on a
// wrong size.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../karpenter-sigs_amd/csrc/ks_tplmask.h"

static size_t r16(size_t b) { return (b + 15) & ~(size_t)15; }

int main() {
  const int ntpls[] = {1, 2, 3, 64, 65}, tws[] = {1, 2, 3, 13, 64};
  int cases = 0;
  for (int NTPL : ntpls)
    for (int TW : tws) {
      // the carve: take(4 * words) then take(4 * NTPL), each rounded up to 16 bytes
      const size_t rows = r16(4 * (size_t)ks::tpl_mask_words(NTPL, TW)), flags = r16(4 * (size_t)NTPL);
      if (ks::tpl_mask_bytes(NTPL, TW) != rows + flags) {
        std::fprintf(stderr, "tpl_mask_plan: bytes %zu != carve %zu (NTPL %d, TW %d)\n", ks::tpl_mask_bytes(NTPL, TW),
                     rows + flags, NTPL, TW);
        return 1;
      }
      std::vector<uint32_t> lds(ks::tpl_mask_bytes(NTPL, TW) / 4, 0u);
      uint32_t* s_tmask = lds.data();
      uint32_t* s_tmv = lds.data() + rows / 4;
      // every instance-type count that ends in this TW, at its chunk edges
      for (int nIT : {32 * (TW - 1) + 1, 32 * TW - 1, 32 * TW}) {
        for (int t = 0; t < NTPL; t++) {
          uint32_t* ic = s_tmask + (size_t)t * 2 * TW;
          uint32_t* of = ic + TW;
          for (int base = 0; base < nIT; base += 64)
            for (uint32_t* dst : {ic, of}) {
              const uint64_t m = ~0ull;
              dst[base >> 5] = (uint32_t)m;
              if ((base >> 5) + 1 < TW) dst[(base >> 5) + 1] = (uint32_t)(m >> 32);
            }
          s_tmv[t] = 1u;
        }
        for (int t = 0; t < NTPL; t++)
          for (int pos = 0; pos < nIT; pos++)
            if (!((s_tmask[(size_t)t * 2 * TW + (pos >> 5)] >> (pos & 31)) & 1u) ||
                !((s_tmask[(size_t)t * 2 * TW + TW + (pos >> 5)] >> (pos & 31)) & 1u)) {
              std::fprintf(stderr, "tpl_mask_plan: bit %d of template %d lost (NTPL %d, TW %d)\n", pos, t, NTPL, TW);
              return 1;
            }
      }
      // the plan's test at its edge: room for the table and 64 claims exactly, and one byte less
      const size_t posB = 16 + 8 * 4, clmB = 16 + 16 * 4 + 4 * (size_t)TW + 4 * 4;
      const size_t need = ks::tpl_mask_bytes(NTPL, TW) + 64 * (posB + clmB);
      if (!ks::tpl_mask_fits(need, NTPL, TW, posB, clmB) || ks::tpl_mask_fits(need - 1, NTPL, TW, posB, clmB) ||
          ks::tpl_mask_fits(need, 0, TW, posB, clmB)) {
        std::fprintf(stderr, "tpl_mask_plan: fit test wrong at its edge (NTPL %d, TW %d)\n", NTPL, TW);
        return 1;
      }
      cases++;
    }
  std::printf("tpl_mask_plan: %d shapes ok\n", cases);
  return 0;
}
