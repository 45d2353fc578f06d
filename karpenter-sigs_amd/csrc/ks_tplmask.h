// ks_tplmask.h — sizes of the LEAN Solve's per-template requirement / offering bitsets (KS_TPL_MASKS; Solver::s_tmask
// and s_tmv in ks_solve.hip) and the plan's test for keeping them.  Plain arithmetic shared by the kernel's LDS carve
// and make_plan, so that a host-only program can check one against the other (scripts/tpl_mask_plan_main.cpp).
#pragma once
#include <cstddef>

namespace ks {

// LDS words of the rows: per template [TW] Intersects, [TW] hasOffering
constexpr int tpl_mask_words(int NTPL, int TW) { return NTPL * 2 * TW; }
// bytes in the plan: the rows, then one flag word per template, each array rounded to 16 bytes as the carve rounds it
constexpr size_t tpl_mask_bytes(int NTPL, int TW) {
  return (((size_t)4 * (size_t)tpl_mask_words(NTPL, TW) + 15) & ~(size_t)15) + (((size_t)4 * (size_t)NTPL + 15) & ~(size_t)15);
}
// The plan keeps the table when, after the instance-type tables, it still leaves room for 64 NodeClaims' position
// and claim state (posB + clmB bytes each) -- the test the instance-type tables themselves pass.
constexpr bool tpl_mask_fits(size_t avail, int NTPL, int TW, size_t posB, size_t clmB) {
  return NTPL > 0 && tpl_mask_bytes(NTPL, TW) + 64 * (posB + clmB) <= avail;
}

}  // namespace ks
