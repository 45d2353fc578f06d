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

#include "ks_disrupt.h"
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

// One claim's row.  t: its template (the caller has tested it against NTPL); opt: its [TW] option words over the
// template's list (cut at the list's length here); rs: its [RSW] requirement record; ctOnly >= 0: an offering is
// also allowed only with that capacity-type value (consolidation's narrowing to spot, consolidation.go:181-188).
// Every lane of the workgroup calls it with the same arguments.  s_kraw: 64 KeyMeta of static LDS; s_dyn:
// launch_lds_bytes of dynamic LDS.
__device__ __forceinline__ void launch_row(const KsDev& D, uint32_t KS_L* s_kraw, unsigned char KS_L* s_dyn, int t,
                                           const uint32_t* __restrict__ opt, const uint32_t* __restrict__ rs, int ctOnly,
                                           const int32_t* __restrict__ name_rank, LaunchRow* __restrict__ row) {
  const KsDims& d = D.d;
  const int tid = (int)threadIdx.x, TW = d.TW, M = 32 * TW, RSW = d.RSW;
  uint64_t KS_L* s_key = (uint64_t KS_L*)s_dyn;            // [M]
  double KS_L* s_price = (double KS_L*)(s_key + M);        // [M]
  int32_t KS_L* s_rank = (int32_t KS_L*)(s_price + M);     // [M]
  int32_t KS_L* s_it = s_rank + M;                         // [M]
  uint32_t KS_L* s_w = (uint32_t KS_L*)(s_it + M);         // [TW] the option words, cut at the template's list
  int32_t KS_L* s_off = (int32_t KS_L*)(s_w + TW);         // [TW + 1] options before each word; [TW]: n
  uint32_t KS_L* s_rec = (uint32_t KS_L*)(s_off + TW + 1); // [RSW] the claim's requirements
  const int tb = D.tpl_it_beg[t], nIT = D.tpl_it_beg[t + 1] - tb;

  for (int i = tid; i < d.NK * (int)(sizeof(KeyMeta) / 4); i += 256) s_kraw[i] = ((const uint32_t KS_G*)D.keys)[i];
  for (int w = tid; w < TW; w += 256) {
    const int left = nIT - 32 * w;
    const uint32_t m = left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : (1u << left) - 1u);
    s_w[w] = opt[w] & m;
  }
  for (int i = tid; i < RSW; i += 256) s_rec[i] = rs[i];
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
      if (ctOnly >= 0 && ct != ctOnly) continue;
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

__global__ __launch_bounds__(256) void k_launch_lists(KsDev D, const int32_t* __restrict__ c_tpl,
                                                      const uint32_t* __restrict__ c_rs, const uint32_t* __restrict__ c_rem,
                                                      const int32_t* __restrict__ order,
                                                      const int32_t* __restrict__ name_rank, int nc,
                                                      LaunchRow* __restrict__ rows) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  const int k = (int)blockIdx.x;
  if (k >= nc) return;  // (uniform over the workgroup)
  const int c = order[k];
  const bool cok = c >= 0 && c < d.Kcap;
  const int t = cok ? c_tpl[c] : -1;
  if (!cok || t < 0 || t >= d.NTPL) return;  // (uniform) the row keeps the host's fill and fails its check
  launch_row(D, (uint32_t KS_L*)s_kraw, (unsigned char KS_L*)s_dyn, t, c_rem + (size_t)c * d.TW,
             c_rs + (size_t)c * d.RSW, -1, name_rank, rows + k);
}

// The launch lists of a consolidation pass: one workgroup per launch slot.  A slot whose record is no Replace (or
// reports a kernel error) returns at once (uniform) and its row keeps the host's fill.  The options are the
// command's: the record's words after filterByPrice, after filterOutSameType for a multi-node prefix (CF_MULTI);
// the requirements are NewNodeClaims[0]'s in the slot's workspace, read as narrowed to capacity type `spot` when
// the record says so (RB_NARROWED).  The claim id is tested against the workspace's claim capacity (its pod count,
// ks_cons.cpp prepare_launch), the template against NTPL.
__global__ __launch_bounds__(256) void k_launch_lists_sims(KsDev D, const KsWork* __restrict__ works,
                                                           const int32_t* __restrict__ recs, int recWords,
                                                           const int32_t* __restrict__ name_rank, int spot, int ns,
                                                           LaunchRow* __restrict__ rows) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  const int k = (int)blockIdx.x;
  if (k >= ns) return;  // (uniform over the workgroup)
  const int32_t* r = recs + (size_t)k * recWords;
  if (r[RF_ACTION] != CA_REPLACE || r[RF_ERROR] != KE_OK) return;  // (uniform)
  const KsWork& W = works[k];
  const int K = W.P > 1 ? W.P : 1;
  const int c = r[RF_CLAIM], t = r[RF_TPL];
  if (c < 0 || c >= K || t < 0 || t >= d.NTPL) return;  // (uniform) the row keeps the host's fill and fails its check
  const uint32_t* opt = (const uint32_t*)r + RF_HDR + ((W.cflags & CF_MULTI) ? 2 : 1) * d.TW;
  launch_row(D, (uint32_t KS_L*)s_kraw, (unsigned char KS_L*)s_dyn, t, opt, (const uint32_t*)W.c_rs + (size_t)c * d.RSW,
             (r[RF_FLAGS] & RB_NARROWED) ? spot : -1, name_rank, rows + k);
}

// The launch lists of a Drift / Expiration pick, from the buffer k_disrupt_pick wrote (ks_disrupt.h): workgroup k
// takes exported claim k.  Nothing to do without a pick, or past the exported claims; every read of `out` lies
// below `cap` words (the pick kernel exported the claims only when they fit).
__global__ __launch_bounds__(256) void k_launch_lists_export(KsDev D, const int32_t* __restrict__ out, int npos, int cap,
                                                             const int32_t* __restrict__ name_rank, int nrows,
                                                             LaunchRow* __restrict__ rows) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  extern __shared__ __attribute__((aligned(16))) unsigned char s_dyn[];
  const int k = (int)blockIdx.x;
  if (k >= nrows || cap < DH_WORDS) return;  // (uniform over the workgroup)
  if (out[DH_PICK] < 0 || k >= out[DH_EXPORTED]) return;  // (uniform)
  const int stride = disrupt_claim_words(d.R, d.TW, d.RSW);
  const long long end = (long long)DH_WORDS + npos + (long long)(k + 1) * stride;
  if (end > (long long)cap) return;  // (uniform)
  const int32_t* cl = out + DH_WORDS + npos + (size_t)k * stride;
  const int t = cl[0];
  if (t < 0 || t >= d.NTPL) return;  // (uniform) the row keeps the host's fill and fails its check
  launch_row(D, (uint32_t KS_L*)s_kraw, (unsigned char KS_L*)s_dyn, t, (const uint32_t*)cl + 3,
             (const uint32_t*)cl + 3 + d.TW + 2 * d.R, -1, name_rank, rows + k);
}

namespace {
// The dynamic LDS of one of the kernels above for this problem; hipErrorInvalidValue when it does not fit.
template <class K> hipError_t launch_lds(K kernel, const KsDev& D, size_t& lds) {
  lds = launch_lds_bytes(D.d.TW, D.d.RSW);
  if (lds > kLaunchMaxLds) return hipErrorInvalidValue;
  if (lds > 48 * 1024) return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  return hipSuccess;
}
}  // namespace

hipError_t launch_lists(const KsDev& D, const KsWork& W, const int32_t* it_name_rank, int nc, LaunchRow* rows,
                        hipStream_t st) {
  if (nc < 1 || !rows || !it_name_rank) return hipErrorInvalidValue;
  size_t lds = 0;
  hipError_t e = launch_lds(k_launch_lists, D, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_launch_lists, dim3((unsigned)nc), dim3(256), lds, st, D, (const int32_t*)W.c_tpl,
                     (const uint32_t*)W.c_rs, (const uint32_t*)W.c_rem, (const int32_t*)W.order, it_name_rank, nc, rows);
  return hipGetLastError();
}

hipError_t launch_lists_sims(const KsDev& D, const KsWork* works, const int32_t* recs, int recWords,
                             const int32_t* it_name_rank, int ns, LaunchRow* rows, hipStream_t st) {
  if (ns < 1 || !rows || !it_name_rank || !works || !recs || recWords < rec_words(D.d.TW)) return hipErrorInvalidValue;
  size_t lds = 0;
  hipError_t e = launch_lds(k_launch_lists_sims, D, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_launch_lists_sims, dim3((unsigned)ns), dim3(256), lds, st, D, works, recs, recWords, it_name_rank,
                     (int)D.d.spotBit, ns, rows);
  return hipGetLastError();
}

hipError_t launch_lists_export(const KsDev& D, const int32_t* out, int npos, int cap, const int32_t* it_name_rank,
                               int nrows, LaunchRow* rows, hipStream_t st) {
  if (nrows < 1 || npos < 1 || cap < DH_WORDS || !rows || !it_name_rank || !out) return hipErrorInvalidValue;
  size_t lds = 0;
  hipError_t e = launch_lds(k_launch_lists_export, D, lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_launch_lists_export, dim3((unsigned)nrows), dim3(256), lds, st, D, out, npos, cap, it_name_rank,
                     nrows, rows);
  return hipGetLastError();
}

}  // namespace ks
