// ks_sort_probe.h — the host side of ks_claim_sort_probe: argument checks and the expected value, Go's
// pdqsort_func (ks_gosort.h) over the caller's (keys, order) with the position arrays regathered from the claim
// tables.  Host-only and free of the HIP runtime, so a stand-alone program can run it under sanitizers
// (scripts/sort_probe_host_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "ks_gosort.h"
#include "ks_problem.h"  // kProbeMaxN
#include "ks_sort_regs.h"

namespace ks {

// nullptr when the arguments are ones the probe accepts, else what is wrong with them
inline const char* sort_probe_check(int mode, int pos, int n, int R, const int32_t* keys, const int32_t* order,
                                    const int32_t* claim_tpl, const int64_t* claim_head, const int32_t* ptpl,
                                    const int64_t* phead) {
  if (n < 0 || n > kProbeMaxN) return "n must be 0 .. kProbeMaxN";
  if (R != 3 && R != 4) return "R must be 3 or 4";
  if (mode != 0 && mode != 1) return "mode must be 0 or 1";
  if (mode == 1 && (pos < 0 || pos >= n)) return "mode 1 needs 0 <= pos < n";
  if (n > 0 && (!keys || !order || !claim_tpl || !claim_head || !ptpl || !phead)) return "null argument";
  for (int j = 0; j < n; j++)
    if (order[j] < 0 || order[j] >= n) return "order holds claim ids 0 .. n - 1";
  return nullptr;
}

// sort.Slice over (keys, order), then ptpl[j] / phead[j][.] of the claim at each position
inline void sort_probe_host(int n, int R, int32_t* keys, int32_t* order, const int32_t* claim_tpl,
                            const int64_t* claim_head, int32_t* ptpl, int64_t* phead) {
  GoSortExact g{GoSort{keys, order}};
  g.run(n);
  for (int j = 0; j < n; j++) {
    const int c = order[j];
    ptpl[j] = claim_tpl[c];
    for (int r = 0; r < R; r++) phead[(size_t)j * R + r] = claim_head[(size_t)c * R + r];
  }
}

// The same from the lane model of the register-copy re-sort (ks_sort_regs.h: sort_regs_model, its how and *path)
inline int sort_probe_model(int n, int R, int32_t* keys, int32_t* order, const int32_t* claim_tpl,
                            const int64_t* claim_head, int32_t* ptpl, int64_t* phead, bool two, int* path) {
  const int how = sort_regs_model(n, keys, order, two, path);
  for (int j = 0; j < n; j++) {
    const int c = order[j];
    ptpl[j] = claim_tpl[c];
    for (int r = 0; r < R; r++) phead[(size_t)j * R + r] = claim_head[(size_t)c * R + r];
  }
  return how;
}

}  // namespace ks
