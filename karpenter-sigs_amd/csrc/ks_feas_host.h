// ks_feas_host.h — the static feasibility matrix on the host (ks_feas_host.cpp): the definitions of DESIGN §3
// "Static feasibility matrix" in plain loops on the host tables, and the arrays one evaluation returns.
#pragma once
#include <cstdint>
#include <vector>

#include "ks_host.h"
#include "ks_problem.h"

namespace ks {

// The five arrays of one evaluation (host copies).
struct StaticFeas {
  int S = 0, NTPL = 0, N = 0, TW = 0, NWN = 0;
  std::vector<uint32_t> tpl_code;     // [S][NTPL] FC_* (FC_NO_IT: | FF_* << 8)
  std::vector<int32_t> tpl_count;     // [S][NTPL] options
  std::vector<uint32_t> tpl_options;  // [S][NTPL][TW] template positions
  std::vector<uint32_t> node_bits;    // [S][NWN]
  std::vector<int32_t> node_count;    // [S]
};

// state -> pod (pod_state0 is a running count)
std::vector<int32_t> state_pods(const Host& h);
// where = 1: plain loops over the host tables through the host side of ks_reqset.h; no HIP call.
void static_feasibility_host(const Host& h, StaticFeas& out);
// The table bytes the two kernels address and the rows they write (DESIGN §3's roofline convention).
void static_feasibility_bytes(const Host& h, const StaticFeas& f, int64_t* read, int64_t* written);

}  // namespace ks
