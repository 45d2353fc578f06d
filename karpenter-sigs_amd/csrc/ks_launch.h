// ks_launch.h — launch lists (ks_launch.hip): NodeClaimTemplate.ToNodeClaim's OrderByPrice and its cut to 100
// instance types (nodeclaimtemplate.go:55-60, types.go:62-79), one row per NewNodeClaim of a Solve.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "ks_problem.h"

namespace ks {

constexpr int kLaunchMax = 100;  // MaxInstanceTypes (nodeclaimtemplate.go:36)

// One NodeClaim's row.  The host fills the buffer with 0xFF bytes before the launch: a slot the kernel does not
// store reads back as -1 / a NaN.
struct LaunchRow {
  int32_t n_options;          // the claim's InstanceTypeOptions
  int32_t n_launch;           // min(n_options, kLaunchMax)
  int32_t its[kLaunchMax];    // instance-type ids in OrderByPrice order
  double prices[kLaunchMax];  // the key's price: the cheapest allowed available offering, DBL_MAX when none
};
static_assert(sizeof(LaunchRow) == 8 + 12 * kLaunchMax, "LaunchRow has no padding");

// LDS bytes k_launch_lists needs for a problem whose longest template list spans TW option words: per option
// slot a 64-bit price key, the price, the name rank and the instance-type id; the claim's option words with their
// running counts; its requirement record.
constexpr size_t launch_lds_bytes(int TW, int RSW) {
  return (size_t)32 * TW * 24 + 4 * (size_t)(2 * TW + 2) + 4 * (size_t)RSW + 16;
}
constexpr size_t kLaunchMaxLds = 160 * 1024 - 2048;  // (the key table is static LDS)

// Rows [0, nc) of `rows` from replica W's final claim state, row k being claim order[k]; nc >= 1, on st.
// hipErrorInvalidValue when the problem's lists do not fit the LDS (launch_lds_bytes above kLaunchMaxLds).
hipError_t launch_lists(const KsDev& D, const KsWork& W, const int32_t* it_name_rank, int nc, LaunchRow* rows,
                        hipStream_t st);

// A consolidation pass's rows (k_launch_lists_sims): row k for launch slot k of `works` / `recs` (ns slots, recWords
// words a record).  A slot whose record is a Replace gets the command's launch list: the options after
// filterByPrice (after filterOutSameType for a multi-node prefix), NewNodeClaims[0]'s requirements, narrowed to spot
// when the record says so.  Every other row keeps the caller's 0xFF fill.
hipError_t launch_lists_sims(const KsDev& D, const KsWork* works, const int32_t* recs, int recWords,
                             const int32_t* it_name_rank, int ns, LaunchRow* rows, hipStream_t st);

// A Drift / Expiration pick's rows (k_launch_lists_export): row k for NodeClaim k of the buffer k_disrupt_pick wrote
// (`out`, cap words, npos positions; ks_disrupt.h), enqueued behind it.  nrows bounds the grid (the plan's bound on
// NodeClaims); rows past the exported claims, and all of them without a pick, keep the caller's 0xFF fill.
hipError_t launch_lists_export(const KsDev& D, const int32_t* out, int npos, int cap, const int32_t* it_name_rank,
                               int nrows, LaunchRow* rows, hipStream_t st);

}  // namespace ks
