// ks_feas.h — launchers of the static feasibility matrix's two kernels (ks_feas.hip; DESIGN §3 "Static
// feasibility matrix"): every relaxation state against every NodeClaimTemplate's instance types and every
// existing node, on the problem's static tables.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

#include "ks_problem.h"

namespace ks {

// Device outputs of one evaluation (all of them device pointers); st_pod: [S] the state's pod.
struct StaticFeasDev {
  const int32_t* st_pod;
  uint32_t* tpl_code;
  int32_t* tpl_count;
  uint32_t* tpl_options;
  uint32_t* node_bits;
  int32_t* node_count;  // zeroed by the caller: k_static_nodes adds to it
};
// LDS the template kernel needs beyond its key table; the caller refuses a problem above the device's limit.
size_t static_templates_lds(const KsDims& d);
void launch_static_templates(const KsDev& D, const StaticFeasDev& o, hipStream_t st);
void launch_static_nodes(const KsDev& D, const StaticFeasDev& o, hipStream_t st);

}  // namespace ks
