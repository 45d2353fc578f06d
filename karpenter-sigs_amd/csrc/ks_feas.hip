// ks_feas.hip — the static feasibility matrix (DESIGN §3 "Static feasibility matrix"): for every relaxation
// state, what Scheduler.add's template phase gives a fresh NodeClaim of each template before any commit
// (scheduler.go:258-285, nodeclaim.go:65-119,225-278) and which existing nodes ExistingNode.Add accepts on
// their initial state (existingnode.go:64-124), topology and volume limits left out.  Both are pure functions
// of the problem's static tables, in the order and with the codes of k_solve's try_templates and node scan
// (ks_solve.hip); ks_feas_host.cpp holds the same definitions in plain loops.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ks_feas.h"
#include "ks_problem.h"
#include "ks_reqset.h"

namespace ks {
namespace {

using DevLayout = ReqLayoutT<const KeyMeta KS_L*, const uint32_t KS_G*, const int64_t KS_G*>;
using LU32 = uint32_t KS_L*;

__device__ __forceinline__ int lane() { return (int)threadIdx.x & (kWave - 1); }
__device__ __forceinline__ uint64_t wballot(bool p) { return __ballot(p ? 1 : 0); }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ bool ub(bool x) { return __builtin_amdgcn_readfirstlane((int)x) != 0; }
// Ordering point for a wave's LDS traffic: its LDS operations execute in order, only the compiler must be kept
// from reordering them.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// The key table staged in LDS once per block (as k_feasibility does) and the layout over it.
__device__ __forceinline__ DevLayout stage_layout(const KsDev& D, uint32_t* s_kraw) {
  const KsDims& d = D.d;
  for (int i = threadIdx.x; i < d.NK * (int)(sizeof(KeyMeta) / 4); i += blockDim.x) s_kraw[i] = ((const uint32_t KS_G*)D.keys)[i];
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
  return L;
}

// filterByRemainingResources (scheduler.go:364-383) of one instance type against the pool's initial remaining
// limits.  pool < 0: no limit pool, every position is a candidate.
__device__ __forceinline__ bool within_limits(const KsDev& D, int it, int pool, uint32_t mask) {
  bool ok = true;
  if (pool >= 0) {
    const int R = D.d.R;
    const int64_t KS_G* cap = D.it_cap + (int64_t)it * R;
    const int64_t KS_G* rem = D.pool_rem0 + (int64_t)pool * R;
    for (int r = 0; r < R; r++) ok &= !((mask >> r) & 1u) | (cap[r] <= rem[r]);
  }
  return ok;
}

}  // namespace

// k_static_templates: one wave per (state, template) row, lanes over the template's positions.  Persistent
// 256-lane blocks, the key table staged once per block, each wave walking rows with a grid stride; the merged
// record (the template's requirements plus the state's) lives in the wave's own LDS scratch.  The instance
// types' records, Allocatable rows and offerings are shared by every row and are read through L2.  Every
// requirement and offering test is the exact one of ks_reqset.h (no position tables), so multi-valued keys and
// irregular positions need no second path.
// Every branch around a store is wave-uniform (made scalar with readfirstlane where the compiler cannot see
// it); the per-lane tests run on a clamped position and are masked by select afterwards (DESIGN §3's rule).
// The option words are stored by lanes 0 and 32 from the ballot, the row's code and count by lane 0 after the
// last uniform branch.  Store indices: row < S * NTPL by the loop bound, word < TW by the loop bound / guard.
__global__ __launch_bounds__(256) void k_static_templates(KsDev D, StaticFeasDev o) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  extern __shared__ __attribute__((aligned(16))) uint32_t s_dyn[];  // [4][RSW] merged records
  const DevLayout L = stage_layout(D, s_kraw);
  const int wave = uni((int)(threadIdx.x >> 6));
  const LU32 mrg = (LU32)s_dyn + wave * d.RSW;
  const int rows = d.S * d.NTPL, R = d.R, TW = d.TW;
  for (int row = (int)blockIdx.x * 4 + wave; row < rows; row += (int)gridDim.x * 4) {
    const int s = row / d.NTPL, t = row - s * d.NTPL;
    const int p = uni(o.st_pod[s]);
    const int tb = uni(D.tpl_it_beg[t]), nIT = uni(D.tpl_it_beg[t + 1]) - tb;
    const int pool = uni(D.tpl_pool[t]);
    const uint32_t pmask = pool >= 0 ? (uint32_t)uni((int)D.pool_mask[pool]) : 0u;
    uint32_t* out = o.tpl_options + (int64_t)row * TW;
    uint32_t code = FC_NONE;
    int cnt = 0;
    bool filled = false;  // the option words of this row are written (uniform)
    // 1) filterByRemainingResources over pool_rem0
    bool anyCand = true;
    if (pool >= 0) {
      uint64_t any = 0;
      for (int base = 0; base < nIT; base += kWave) {
        const int pos = base + lane();
        const int pc = pos < nIT ? pos : nIT - 1;
        any |= wballot(within_limits(D, D.tpl_its[tb + pc], pool, pmask) & (pos < nIT));
      }
      anyCand = any != 0;
    }
    if (!anyCand) {
      code = FC_LIMITS;
    } else if (!ub((D.st_toltpl[s] >> t) & 1ull)) {  // 2) the template's taints
      code = FC_TAINTS;
    } else {
      // 3) Compatible(template, state, allowWK), then Requirements.Add.  Every lane runs the same record
      // algebra on the wave's record: wave-wide loads and stores of uniform values.
      const uint32_t KS_G* T = D.tpl_rs + (int64_t)t * d.RSW;
      for (int i = lane(); i < d.RSW; i += kWave) mrg[i] = T[i];
      wsync();
      bool ok = true;
      if (ub((D.st_flags[s] & SF_HAS_KEYS) != 0)) {
        const uint32_t KS_G* X = D.st_rs + (int64_t)s * d.RSW;
        ok = ub(rs_compatible(L, mrg, X, d.allowWK));
        if (ok) rs_add(L, mrg, X);
        wsync();
      }
      if (!ok) {
        code = FC_COMPAT;
      } else {
        // 4) the instance-type filter: Intersects, Fits(daemon overhead + pod), an offering
        int64_t req[kMaxR];
#pragma unroll
        for (int r = 0; r < kMaxR; r++) {
          if (r >= R) break;
          req[r] = D.tpl_daemon[(int64_t)t * R + r] + D.pod_req[(int64_t)p * R + r];
        }
        uint32_t flags = 0;
        for (int base = 0; base < TW * 32; base += kWave) {
          const int pos = base + lane();
          const bool in = pos < nIT;
          const int pc = in ? pos : (nIT > 0 ? nIT - 1 : 0);
          bool ic = false, fi = false, of = false;
          if (nIT > 0) {  // (uniform)
            const int it = D.tpl_its[tb + pc];
            const bool cand = in & within_limits(D, it, pool, pmask);
            ic = rs_intersects(L, D.it_rs + (int64_t)it * d.RSW, mrg);
            const int64_t KS_G* al = D.it_alloc + (int64_t)it * R;  // resources.go:162-175, as fits_pos
            fi = true;
#pragma unroll
            for (int r = 0; r < kMaxR; r++) {
              if (r >= R) break;
              const int64_t a = al[r];
              fi &= (a >= 0) & (req[r] <= a);
            }
            const int ob = D.it_off_beg[it], oe = D.it_off_beg[it + 1];  // nodeclaim.go:270-278
            for (int q = ob; q < oe; q++)
              of |= rs_member(L, mrg, d.zoneKey, D.off_zone[q]) && rs_member(L, mrg, d.ctKey, D.off_ct[q]);
            ic &= cand;
            fi &= cand;
            of &= cand;
          }
          if (wballot(ic)) flags |= FF_REQ;
          if (wballot(fi)) flags |= FF_FITS;
          if (wballot(of)) flags |= FF_OFF;
          if (wballot(ic && fi && !of)) flags |= FF_REQ_FITS;
          if (wballot(ic && of && !fi)) flags |= FF_REQ_OFF;
          if (wballot(fi && of && !ic)) flags |= FF_FITS_OFF;
          const uint64_t m = wballot(ic && fi && of);
          cnt += __popcll(m);
          const int w = base >> 5;  // < TW by the loop bound
          if (lane() == 0) out[w] = (uint32_t)m;
          if (lane() == 32 && w + 1 < TW) out[w + 1] = (uint32_t)(m >> 32);
        }
        filled = true;
        if (cnt == 0) code = FC_NO_IT | (flags << 8);
      }
    }
    if (!filled)
      for (int w = lane(); w < TW; w += kWave) out[w] = 0;
    if (lane() == 0) {
      o.tpl_code[row] = code;
      o.tpl_count[row] = cnt;
    }
  }
}

// k_static_nodes: one thread per (state, node), a block of 256 nodes of one state.  Lanes test their node
// against the same state (taints, host ports, Fits with the negative-total rule, strict Compatible); a ballot
// packs 64 node bits, lanes 0 and 32 store one word each, and the wave adds its popcount to node_count[s]
// with one atomic.  A pod whose GetVolumes fails (PF_VOLERR) has zero rows (existingnode.go:70-73).
__global__ __launch_bounds__(256) void k_static_nodes(KsDev D, StaticFeasDev o, int nbx) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
  const DevLayout L = stage_layout(D, s_kraw);
  const int s = (int)blockIdx.x / nbx, bx = (int)blockIdx.x - s * nbx;  // s < S by the grid size
  const int p = uni(o.st_pod[s]);
  const int R = d.R;
  const uint32_t KS_G* X = D.st_rs + (int64_t)s * d.RSW;
  const uint64_t t0 = D.st_tol[2 * s], t1 = D.st_tol[2 * s + 1];
  const uint64_t hpc = D.pod_hpc[p];
  const bool keys = (D.st_flags[s] & SF_HAS_KEYS) != 0;
  const bool dead = (D.pod_flags[p] & PF_VOLERR) != 0;
  const int NWN = (d.N + 31) >> 5;
  const int n = bx * 256 + (int)threadIdx.x;  // a wave's 64 nodes start at a multiple of 64
  const int nc = n < d.N ? n : d.N - 1;       // (N > 0: the launcher skips an empty node list)
  const uint64_t KS_G* tp = D.n_taint + 2 * (int64_t)nc;
  bool ok = (n < d.N) & !dead;
  ok &= ((tp[0] & ~t0) | (tp[1] & ~t1)) == 0;  // Taints.Tolerates
  ok &= (D.n_hp0[nc] & hpc) == 0;              // HostPortUsage.Conflicts (the pod's own entries left out)
  const int64_t KS_G* av = D.n_avail + (int64_t)nc * R;
  const int64_t KS_G* rq = D.n_req0 + (int64_t)nc * R;
  const int64_t KS_G* pr = D.pod_req + (int64_t)p * R;
  for (int r = 0; r < R; r++) {  // Fits(requests + pod, Available())
    const int64_t a = av[r];
    ok &= (a >= 0) & (rq[r] + pr[r] <= a);
  }
  if (keys) ok = ok & rs_compatible(L, D.n_rs0 + (int64_t)nc * d.RSW, X, 0);  // (a select: ok keeps its masks)
  const uint64_t b = wballot(ok);
  const int w = (n - lane()) >> 5;  // this wave's first word
  uint32_t* out = o.node_bits + (int64_t)s * NWN;
  if (lane() == 0 && w < NWN) out[w] = (uint32_t)b;
  if (lane() == 32 && w + 1 < NWN) out[w + 1] = (uint32_t)(b >> 32);
  if (lane() == 0 && b) atomicAdd(o.node_count + s, __popcll(b));
}

size_t static_templates_lds(const KsDims& d) { return 4 * (size_t)d.RSW * sizeof(uint32_t); }

void launch_static_templates(const KsDev& D, const StaticFeasDev& o, hipStream_t st) {
  const int rows = D.d.S * D.d.NTPL;
  if (rows <= 0) return;
  const int blocks = std::min(4096, (rows + 3) / 4);
  hipLaunchKernelGGL(k_static_templates, dim3(blocks), dim3(256), static_templates_lds(D.d), st, D, o);
}

void launch_static_nodes(const KsDev& D, const StaticFeasDev& o, hipStream_t st) {
  if (D.d.S <= 0 || D.d.N <= 0) return;
  const int nbx = (D.d.N + 255) / 256;
  hipLaunchKernelGGL(k_static_nodes, dim3(D.d.S * nbx), dim3(256), 0, st, D, o, nbx);
}

}  // namespace ks
