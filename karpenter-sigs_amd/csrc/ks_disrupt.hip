// ks_disrupt.hip — Drift / Expiration (drift.go:77-118, expiration.go:83-120) over a method's launch of
// single-candidate simulations: the sequential choice and the chosen simulation's NewNodeClaims in one launch.
//
// The method's candidates are simulated like a pass's single-node candidates (k_solve<SIM>, ks_cons.cpp).  The
// command is the first candidate, in the method's order, whose simulation scheduled every non-pending pod; its
// replacements are every NodeClaim of that simulation.  k_disrupt_pick finds that position and copies the claim
// state the simulation left in its workspace (the SIM epilogue's write-back, ks_solve_body.inc; c_tpl / c_host /
// c_rs from claim creation and every later narrowing) into one buffer, so the host makes one copy instead of a
// read of every record followed by dependent copies of order, c_tpl, c_host, c_rem, c_req and c_rs.
#include <hip/hip_runtime.h>

#include "ks_disrupt.h"

namespace ks {

__global__ __launch_bounds__(256) void k_disrupt_pick(const int32_t* __restrict__ recs, int recWords,
                                                      const KsWork* __restrict__ works, const int32_t* __restrict__ slot,
                                                      int npos, int R, int TW, int RSW, int32_t* __restrict__ out,
                                                      int cap) {
  __shared__ int s_pick[4], s_err[4];
  const int tid = threadIdx.x, wave = tid >> 6;
  // phase 1: the first schedulable position and the first kernel error
  int wpick = kNoPos, werr = kNoPos;  // wave-uniform
  for (int base = 0; base < npos; base += 256) {
    const int i = base + tid;
    const bool in = i < npos;
    const int32_t* r = recs + (size_t)slot[in ? i : 0] * recWords;
    const int flags = r[RF_FLAGS], ncl = r[RF_NCLAIMS], e = r[RF_ERROR];
    const bool ok = in && e == KE_OK && (flags & RB_ALL_SCHEDULED) != 0;
    const bool bad = in && e != KE_OK;
    if (in && DH_WORDS + i < cap) out[DH_WORDS + i] = (ncl << 8) | (flags & 0xff);
    const unsigned long long bo = __ballot(ok ? 1 : 0), bb = __ballot(bad ? 1 : 0);
    const int fo = bo ? base + (wave << 6) + (int)__builtin_ctzll(bo) : kNoPos;
    const int fb = bb ? base + (wave << 6) + (int)__builtin_ctzll(bb) : kNoPos;
    wpick = fo < wpick ? fo : wpick;
    werr = fb < werr ? fb : werr;
  }
  s_pick[wave] = wpick;  // wave-wide stores of wave-uniform values
  s_err[wave] = werr;
  __syncthreads();
  int pick = s_pick[0], errp = s_err[0];
#pragma unroll
  for (int q = 1; q < 4; q++) {
    pick = s_pick[q] < pick ? s_pick[q] : pick;
    errp = s_err[q] < errp ? s_err[q] : errp;
  }
  // phase 2: the picked simulation's NodeClaims
  const bool has = pick != kNoPos;
  const int ps = slot[has ? pick : 0];
  const KsWork& W = works[ps];
  const int K = W.P > 1 ? W.P : 1;  // claim capacity of the workspace (ks_cons.cpp prepare_launch)
  int nclaims = has ? (int)W.counters[CT_NCLAIMS] : 0;
  const int nlog = has ? (int)W.counters[CT_NLOG] : 0;
  nclaims = nclaims < 0 ? 0 : (nclaims > K ? K : nclaims);
  const int stride = 3 + TW + 2 * R + RSW;
  const long long need = (long long)DH_WORDS + npos + (long long)nclaims * stride;
  const bool fits = need <= (long long)cap;
  const int nexp = fits ? nclaims : 0;
  const int cbase = DH_WORDS + npos;
  int anyBad = 0;
  const int32_t KS_G* req32 = (const int32_t KS_G*)W.c_req;
  for (int w = tid; w < nexp * stride; w += 256) {
    const int k = w / stride, f = w - k * stride;
    int c = W.order[k];
    const bool cok = c >= 0 && c < K;
    anyBad |= cok ? 0 : 1;
    c = cok ? c : 0;
    int v;
    if (f == 0) {
      v = W.c_tpl[c];
    } else if (f == 1) {
      v = W.c_host[c];
    } else if (f == 2) {
      v = 0;
      for (int t = 0; t < TW; t++) v += __popc(W.c_rem[(size_t)c * TW + t]);
    } else if (f < 3 + TW) {
      v = (int)W.c_rem[(size_t)c * TW + (f - 3)];
    } else if (f < 3 + TW + 2 * R) {
      v = req32[(size_t)c * 2 * R + (f - 3 - TW)];
    } else {
      v = (int)W.c_rs[(size_t)c * RSW + (f - 3 - TW - 2 * R)];
    }
    out[cbase + w] = v;  // cbase + w < need <= cap
  }
  const int badAll = __syncthreads_or(anyBad);
  const int ecode = recs[(size_t)slot[errp != kNoPos ? errp : 0] * recWords + RF_ERROR];
  if (cap >= DH_WORDS && tid < DH_WORDS) {
    int v = 0;
    v = tid == DH_PICK ? (has ? pick : -1) : v;
    v = tid == DH_ERRPOS ? (errp != kNoPos ? errp : -1) : v;
    v = tid == DH_ERR ? (errp != kNoPos ? ecode : 0) : v;
    v = tid == DH_NCLAIMS ? nclaims : v;
    v = tid == DH_NLOG ? nlog : v;
    v = tid == DH_NEED ? (int)(need > 0x7fffffffLL ? 0x7fffffffLL : need) : v;
    v = tid == DH_BAD ? (badAll ? 1 : 0) : v;
    v = tid == DH_EXPORTED ? nexp : v;
    out[tid] = v;
  }
}

hipError_t disrupt_pick(const int32_t* recs, int recWords, const KsWork* works, const int32_t* slot, int npos, int R,
                        int TW, int RSW, int32_t* out, int cap, hipStream_t st) {
  if (npos <= 0 || cap < DH_WORDS) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_disrupt_pick, dim3(1), dim3(256), 0, st, recs, recWords, works, slot, npos, R, TW, RSW, out, cap);
  return hipGetLastError();
}

}  // namespace ks
