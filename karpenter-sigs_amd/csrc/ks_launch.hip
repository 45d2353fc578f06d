// ks_launch.hip — launch lists: what NodeClaimTemplate.ToNodeClaim (nodeclaimtemplate.go:55-60) hands the cloud
// provider for every NewNodeClaim of a Solve: InstanceTypeOptions.OrderByPrice(requirements) (types.go:62-79) cut to
// its first 100 entries.  An option's price is its cheapest available offering that the claim's zone and
// capacity-type requirements allow (Offerings.Available().Requirements(reqs).Cheapest(), types.go:147-166),
// math.MaxFloat64 when there is none; equal prices are ordered by name.
//
// k_launch_lists: one 256-lane workgroup per NodeClaim, reading the claim state k_solve left in the workspace
// (c_tpl, c_rs, c_rem through `order`) and the problem's offering tables.  The claim's options are compacted into
// LDS slots with their key (price folded to an order-preserving 64-bit integer, name rank); an option's place in
// the order is the number of options with a smaller key, counted against the LDS copy (every lane of a wave reads
// the same slot: a broadcast), so no sort runs and the result does not depend on a sorting network's stability.
// Stores: LDS slot idx < n <= 32 * TW by construction of the running counts; row k < nc by the grid; its / prices
// slot pos tested against kLaunchMax.  A claim or template id outside its table leaves the row as the host filled it.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "ks_launch.h"
#include "ks_problem.h"
#include "ks_reqset.h"

namespace ks {
namespace {

using DevLayout = ReqLayoutT<const KeyMeta KS_L*, const uint32_t KS_G*, const int64_t KS_G*>;

// Go's float64 order as an unsigned integer order; -0.0 == +0.0 in Go, so both take +0.0's key and the name decides.
__device__ __forceinline__ uint64_t price_key(double p) {
  uint64_t u = (uint64_t)__double_as_longlong(p);
  u = p == 0.0 ? 0ull : u;
  return (u >> 63) ? ~u : (u | (1ull << 63));
}

}  // namespace

__global__ __launch_bounds__(256) void k_launch_lists(KsDev D, const int32_t* __restrict__ c_tpl,
                                                      const uint32_t* __restrict__ c_rs, const uint32_t* __restrict__ c_rem,
                                                      const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ name_rank, int nc,
                                                      LaunchRow* __restrict__ rows) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  const int tid = (int)threadIdx.x, TW = d.TW, M = 32 * TW, RSW = d.RSW;
  const int k = (int)blockIdx.x;
  if (k >= nc) return;  // (uniform over the workgroup)
  uint64_t KS_L* s_key = (uint64_t KS_L*)s_dyn;            // [M]
  double KS_L* s_price = (double KS_L*)(s_key + M);        // [M]
  int32_t KS_L* s_rank = (int32_t KS_L*)(s_price + M);     // [M]
  int32_t KS_L* s_it = s_rank + M;                         // [M]
  uint32_t KS_L* s_w = (uint32_t KS_L*)(s_it + M);         // [TW] the option words, cut at the template's list
  int32_t KS_L* s_off = (int32_t KS_L*)(s_w + TW);         // [TW + 1] options before each word; [TW]: n
  uint32_t KS_L* s_rec = (uint32_t KS_L*)(s_off + TW + 1); // [RSW] the claim's requirements

  const int c = order[k];
  const bool cok = c >= 0 && c < d.Kcap;
  const int t = cok ? c_tpl[c] : -1;
  if (!cok || t < 0 || t >= d.NTPL) return;  // (uniform) the row keeps the host's fill and fails its check
  const int tb = D.tpl_it_beg[t], nIT = D.tpl_it_beg[t + 1] - tb;

  for (int i = tid; i < d.NK * (int)(sizeof(KeyMeta) / 4); i += 256) s_kraw[i] = ((const uint32_t KS_G*)D.keys)[i];
  for (int w = tid; w < TW; w += 256) {
    const int left = nIT - 32 * w;
    const uint32_t m = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << left) - 1u);
    s_w[w] = c_rem[(size_t)c * TW + w] & m;
  }
  for (int i = tid; i < RSW; i += 256) s_rec[i] = c_rs[(size_t)c * RSW + i];
  __syncthreads();
  DevLayout L;
  L.nkeys = d.NK;
  L.W = d.W;
  L.NB = d.NB;
  L.HDR = d.HDR;
  L.RSW = d.RSW;
  L.keys = (const KeyMeta KS_L*)s_kraw;
  L.wordValid = D.wordValid;
  L.vIsInt = D.vIsInt;
  L.vInt = D.vInt;

  // 1) the options' slots: an exclusive scan of the words' popcounts (wave 0, 64 words a step)
  if (tid < kWave) {
    int carry = 0;
    for (int base = 0; base < TW; base += kWave) {
      const int w = base + tid;
      const int cnt = w < TW ? __popc(s_w[w]) : 0;
      int incl = cnt;
#pragma unroll
      for (int s = 1; s < kWave; s <<= 1) {
        const int up = __shfl_up(incl, s, kWave);
        incl += tid >= s ? up : 0;
      }
      if (w < TW) s_off[w] = carry + incl - cnt;
      carry += __shfl(incl, kWave - 1, kWave);
    }
    if (tid == 0) s_off[TW] = carry;
  }
  __syncthreads();
  const int n = s_off[TW];  // <= nIT <= M

  // 2) price and key of every option
  const int zoneKey = d.zoneKey, ctKey = d.ctKey;
  const int zoneNv = L.keys[zoneKey].nv, ctNv = L.keys[ctKey].nv;
  for (int p = tid; p < M; p += 256) {
    const uint32_t w = s_w[p >> 5];
    if (!((w >> (p & 31)) & 1u)) continue;
    const int idx = s_off[p >> 5] + __popc(w & ((1u << (p & 31)) - 1u));
    const int it = D.tpl_its[tb + p];  // p < nIT: the words are cut there
    const bool iok = it >= 0 && it < d.T;
    const int itc = iok ? it : 0;
    double best = DBL_MAX;
    bool any = false;
    const int oe = iok ? D.it_off_beg[itc + 1] : 0;
    for (int o = iok ? D.it_off_beg[itc] : 0; o < oe; o++) {
      const int z = D.off_zone[o], ct = D.off_ct[o];
      if (z < 0 || z >= zoneNv || ct < 0 || ct >= ctNv) continue;
      if (!rs_member(L, s_rec, zoneKey, z) || !rs_member(L, s_rec, ctKey, ct)) continue;
      const double pr = D.off_price[o];
      best = (!any || pr < best) ? pr : best;
      any = true;
    }
    if (idx >= 0 && idx < n) {
      s_key[idx] = price_key(best);
      s_price[idx] = best;
      s_rank[idx] = name_rank[itc];
      s_it[idx] = iok ? it : -1;
    }
  }
  __syncthreads();

  // 3) rank by counting, the first kLaunchMax stored
  LaunchRow* row = rows + k;
  for (int i = tid; i < n; i += 256) {
    const uint64_t ki = s_key[i];
    const int ri = s_rank[i];
    int pos = 0;
    for (int j = 0; j < n; j++) {
      const uint64_t kj = s_key[j];
      pos += (kj < ki) | ((kj == ki) & (s_rank[j] < ri));
    }
    if (pos >= 0 && pos < kLaunchMax) {
      row->its[pos] = s_it[i];
      row->prices[pos] = s_price[i];
    }
  }
  if (tid < 2) ((int32_t*)row)[tid] = tid == 0 ? n : (n < kLaunchMax ? n : kLaunchMax);  // n_options, n_launch
}

hipError_t launch_lists(const KsDev& D, const KsWork& W, const int32_t* it_name_rank, int nc, LaunchRow* rows,
                        hipStream_t st) {
  if (nc < 1 || !rows || !it_name_rank) return hipErrorInvalidValue;
  const size_t lds = launch_lds_bytes(D.d.TW, D.d.RSW);
  if (lds > kLaunchMaxLds) return hipErrorInvalidValue;
  if (lds > 48 * 1024) {
    hipError_t e = hipFuncSetAttribute((const void*)k_launch_lists, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_launch_lists, dim3((unsigned)nc), dim3(256), lds, st, D, (const int32_t*)W.c_tpl,
                     (const uint32_t*)W.c_rs, (const uint32_t*)W.c_rem, (const int32_t*)W.order, it_name_rank, nc, rows);
  return hipGetLastError();
}

}  // namespace ks
