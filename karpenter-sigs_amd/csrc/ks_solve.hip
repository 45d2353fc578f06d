// ks_solve.hip — MI355X (gfx950) kernels for Scheduler.Solve.
//
// One Solve = one 64-lane wavefront (one workgroup).  The reference's Solve is a sequential commit
// chain (scheduler.go:140-189: every placement depends on all earlier ones), so the chain stays in
// one wave with wave-uniform control flow and no inter-wave synchronisation; the data-parallel
// parts of each step map onto the 64 lanes:
//   - existing-node first-fit (scheduler.go:240-244)   lane per node, ballot + ffs picks the first
//   - in-flight NodeClaim scan (scheduler.go:250-254)  lane per sorted position: a quick reject
//     (template taints, pod <= max Allocatable - requests, Compatible) from position-indexed
//     arrays, then a wave-cooperative NodeClaim.Add on candidates in order (nodeclaim.go:65-119)
//   - instance-type filter (nodeclaim.go:225-260)      lane per template IT position, ballots build
//     the remaining-options bitset and the six filterResults flags in one pass
//   - new NodeClaim per template (scheduler.go:258-283) incl. limits (filterByRemainingResources,
//     subtractMax)
// When a pod leaves a claim's requirements unchanged (resource-only pods), NodeClaim.Add's option
// filter reduces to Fits on growing requests, so the options it drops are a prefix of each
// resource's Allocatable-ascending order: a per-claim threshold per resource advances over that
// order and clears exactly the dropped options (no scan of the surviving ones).
// Latency is the bound (the chain is sequential), so everything a step touches lives in LDS or
// VGPRs: the 64-pod queue window (one lane per entry, read with readlane), the claim order, pod
// counts and quick-reject headroom per position, each claim's template / requests / max-Allocatable
// / options bitset / thresholds (for the first Plan::KL claims), the templates' Allocatable tables
// and the remaining NodePool limits.  Pointers carry explicit address spaces (ks_problem.h), so no
// access is a flat access.  Lanes never hand data to each other through HBM except at the window
// refill (behind one release fence, read with sc1 loads that bypass the L1).  HBM holds the cold
// state (requirement records, existing nodes, overflow claims) and the write-only commit log.
// Independent Solves (replicas, consolidation simulations) are independent workgroups, so a launch
// of thousands of them fills the 256 CUs.  Nothing here is a dense contraction: no MFMA.
#include <hip/hip_runtime.h>

#ifndef KS_FM_OFF
#define KS_FM_OFF 0
#endif
#ifndef KS_TU
#define KS_TU 0
#endif
#ifndef KS_RUN_MIN  // shortest run of identical pods the simulation fast path places in one step
#define KS_RUN_MIN 3
#endif
#ifndef KS_NODE_K  // existing nodes per lane per step of the first-fit scan beyond the register window
#define KS_NODE_K 2
#endif
#ifndef KS_SORT_LANE0  // 1: the claim re-sort's exact pdqsort on lane 0 (the round-2 form)
#define KS_SORT_LANE0 0
#endif
#ifndef KS_SORT_LEAF  // LEAN Solve: the exact re-sort's frames of <= 12 entries by stable rank on the wave (0: insertionSort on lane 0)
#define KS_SORT_LEAF 1
#endif
#ifndef KS_CLAIM_RUNS  // LEAN Solve: runs of identical pods placed on one NodeClaim in one step
#define KS_CLAIM_RUNS 1
#endif
#ifndef KS_RUN_CROSS  // those runs stay on their NodeClaim across the re-sorts inside a step (0: end at each)
#define KS_RUN_CROSS 1
#endif
#ifndef KS_RUN_FRONT  // their capacity from the template's Pareto-maximal instance types (0: from every remaining option)
#define KS_RUN_FRONT 1
#endif
// LEAN Solve: 1 composes a run's closed-form crossings into one deferred move of its claim (0: each moves and
// regathers).  Measured on C2 at -0.018 ms of 6.85 (-0.077 in an earlier session), under the round's margin of three
// spreads, and at +0.013 ms of 0.322 on the C1 kernel: off
#ifndef KS_RUN_FUSE
#define KS_RUN_FUSE 0
#endif
// LEAN Solve: 1 moves the closed form's block by shifting the four position arrays from registers, its reads
// issued together (0: pis_move, then a regather of s_ptpl / s_phead through the claims).  Round 11 measured it on C2
// at -0.066 ms of 6.74 with choosePivot's samples issued inside it, under that round's margin: off.  On top of
// KS_PIVOT_ARITH (no samples: K, the next key and 256 keys in one batch) it measured -0.179 ms of 5.476, every run
// faster, against a margin of 0.060 ms (round 17): on
#ifndef KS_CLOSED_SHIFT
#define KS_CLOSED_SHIFT 1
#endif
// LEAN Solve: 1 takes choosePivot's hint at the top frame of a re-sort after a count increment at `pos` from n and
// pos alone, with no sample read: for n >= 50 and a confirmed descent at pos the hint is "increasing" exactly when
// pos is none of l-1, l, 2l-1, 2l, 3l-1, 3l (l = n/4), and the pivot is then 2l (DESIGN §3,
// tests/test_pivot_arith_model.py).  Anything else samples as before (0: always samples).
// KS_PIVOT_ARITH_CHECK=1: a diagnostic build that samples as well and counts disagreements (`pivotArithDiff`)
#ifndef KS_PIVOT_ARITH
#define KS_PIVOT_ARITH 1
#endif
#ifndef KS_PIVOT_ARITH_CHECK
#define KS_PIVOT_ARITH_CHECK 0
#endif
// LEAN Solve: 1 lets a run that crossed by the closed form re-test claim_quick only on the entries its claim was
// lifted over, [old position, new position), when no position of this step passed the quick test and failed
// claim_full (0: every position before the new one).  Measured on C2 at +0.018 ms of 5.297 (-0.030 ms of 5.45 in a
// session without the register shift), under the margins of 0.057 and 0.051 ms (round 17): off
#ifndef KS_CROSS_QUICK_FROM
#define KS_CROSS_QUICK_FROM 0
#endif
// LEAN Solve: 1 re-sorts after an appended claim at n >= 50 by its closed form: the new entry goes to the end of the
// counts not above its own, the entries behind move one place right in all four position arrays (0: choosePivot,
// partialInsertionSort and a regather, as before).  Measured on C2 at -0.124 ms of 5.297, every run faster,
// against a margin of 0.075 ms.  It ships off all the same: these re-sorts then are neither closed-form (sortsClosed,
// pinned) nor general ones on the register copy, and tests/test_sort_regs_gpu.py pins sortsRegs + sortRegsOver ==
// sortsWithDescent - sortsClosed (round 17).  scripts/variant_check.sh runs a build with it on
#ifndef KS_APPEND_CLOSED
#define KS_APPEND_CLOSED 0
#endif
#ifndef KS_SORT_CLOSED  // the claim re-sort's closed form at a single count crossing: 0 off, 1 LEAN Solve, 2 every Solve
#define KS_SORT_CLOSED 1
#endif
#ifndef KS_SORT_OUTLINE  // the general claim re-sort as one out-of-line function per kernel (0: inlined at both call sites)
#define KS_SORT_OUTLINE 1
#endif
// LEAN Solve: the general claim re-sort of up to 128 claims runs on a copy held in registers (ks_sort_regs.h) and
// stores it once; anything else, or a failed invariant, leaves the arrays to the LDS code (0: the LDS code alone).
// KS_SORT_REGS_N64: 1 restricts it to n <= 64, one register pair per lane (0: 128, two pairs).  Measured on C2
// against 6.519 ms: 6.218 ms with the 64-entry form, 6.411 ms with the 128-entry one, whose every step pays for the
// second pair: the 64-entry form ships, 65 claims and more stay with the LDS code
#ifndef KS_SORT_REGS
#define KS_SORT_REGS 1
#endif
#ifndef KS_SORT_REGS_N64
#define KS_SORT_REGS_N64 1
#endif
#ifndef KS_TPL_MEMO  // LEAN Solve: a NewNodeClaim reuses what the last one derived from the same template, state, requests
#define KS_TPL_MEMO 1
#endif
// LEAN Solve: 1 issues a run's queue loads for the commit log ahead of its stores (0: 64 per load).  Measured on
// C2 at -0.09 ms of 7.55, under the round's margin of three spreads: off
#ifndef KS_LOG_AHEAD
#define KS_LOG_AHEAD 0
#endif
// LEAN Solve: 1 lets a NewNodeClaim that misses the memo read its template's requirement-compatible / has-offering
// bitsets from LDS, kept by the template's first derivation in this Solve (0: derives them again).  Measured on C2 at
// -0.154 and -0.125 ms of 6.50 in two sessions, all eight runs faster, under the sessions' margins of three spreads
// (0.231 and 0.147 ms): off
#ifndef KS_TPL_MASKS
#define KS_TPL_MASKS 0
#endif
// LEAN Solve: 1 lets a NewNodeClaim that misses the memo take the record k_fresh_claims wrote for (the pod's request
// class, the template) once per handle, instead of deriving it on the one-wave chain (0: derives it, as before).
// Compiled out with KS_TPL_MASKS=1, whose variant build measures the masks' path alone.
#ifndef KS_TPL_TABLE
#define KS_TPL_TABLE 1
#endif
// Self-check build: a NewNodeClaim that would take a record derives it as well and compares every word; a mismatch
// ends the Solve with KE_TPL_TABLE
#ifndef KS_TPL_TABLE_CHECK
#define KS_TPL_TABLE_CHECK 0
#endif
// LEAN Solve: a run past the queue window, while the queue is still NewQueue's order, logs one record and
// k_log_expand writes its per-pod entries after the Solve (0: the wave reads the pods back, 64 per load)
#ifndef KS_LOG_RUNS
#define KS_LOG_RUNS 1
#endif
// LEAN Solve: a pod that exceeds the headroom commit_claim just stored for its claim's position (max Allocatable -
// requests, the quick test's upper bound for every remaining option) in some resource fits none of them a second
// time: the run's capacity is 0 without a claim_run_cap call (0: the call is always made)
#ifndef KS_CAP_BOUND
#define KS_CAP_BOUND 1
#endif
// LEAN Solve: 1 lets claim_full's threshold advance issue the first 64-entry chunk of every resource together (the
// sorted Allocatables, their positions, the option-bit clears, the ballots) instead of resource after resource; a
// resource that dropped all 64 goes on in the per-resource loop (0: that loop alone).  Measured on C2 at +0.072 ms
// of 5.8985 (four runs each, every run slower than every run without it): off
#ifndef KS_THR_BATCH
#define KS_THR_BATCH 0
#endif
// LEAN Solve: 1 lets a popped pod skip the existing-node phase when the pod before it landed on a NodeClaim and is
// identical to it by the claim runs' identity (0: every popped pod scans the nodes)
#ifndef KS_RUN_CHAIN
#define KS_RUN_CHAIN 0
#endif

#include "ks_gosort.h"
#include "ks_problem.h"
#include "ks_reqset.h"
#include "ks_sort_regs.h"
#include "ks_tplmask.h"

namespace ks {

using LI32 = int32_t KS_L*;
using LI64 = int64_t KS_L*;
using LU32 = uint32_t KS_L*;
using LU64 = uint64_t KS_L*;
using GI32 = int32_t KS_G*;
using GI64 = int64_t KS_G*;
using GU32 = uint32_t KS_G*;
using DevLayout = ReqLayoutT<const KeyMeta KS_L*, const uint32_t KS_G*, const int64_t KS_G*>;
// Topology-group sets of the popped pod kept in LDS beyond word 0 (Solver::s_gw rows)
enum GroupSet : int { GS_MASK = 0, GS_SEL, GS_INV, GS_ACT, GS_N };

__device__ __forceinline__ int lane() { return (int)threadIdx.x & (kWave - 1); }
__device__ __forceinline__ uint64_t wballot(bool p) { return __ballot(p ? 1 : 0); }
__device__ __forceinline__ int ctz64(uint64_t m) { return __builtin_ctzll(m); }
__device__ __forceinline__ int popc64(uint64_t m) { return __popcll(m); }
__device__ __forceinline__ int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
// A wave-uniform branch condition.  The commit chain's control flow is uniform by construction, but
// the compiler cannot prove it for values that pass through LDS atomics or lane-indexed loads; a
// condition it believes divergent turns the whole Solve loop into exec-masked code (every loop-carried
// scalar in a VGPR, mask bookkeeping spilled to VGPR lanes).  readfirstlane makes the branch scalar.
__device__ __forceinline__ bool ub(bool x) { return __builtin_amdgcn_readfirstlane((int)x) != 0; }
__device__ __forceinline__ int64_t uni64(int64_t x) {
  return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(x >> 32)) << 32) |
                   (uint32_t)__builtin_amdgcn_readfirstlane((int)x));
}
__device__ __forceinline__ int rdl(int x, int l) { return __builtin_amdgcn_readlane(x, l); }
__device__ __forceinline__ int64_t rdl64(int64_t x, int l) {
  return (int64_t)(((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), l) << 32) |
                   (uint32_t)__builtin_amdgcn_readlane((int)x, l));
}
// Ordering point for LDS traffic between the lanes of the (single) wave: the wave's LDS operations
// execute in order, so only the compiler must be kept from reordering; no s_waitcnt, no s_barrier.
__device__ __forceinline__ void wsync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
// HBM hand-off point (rare paths): every outstanding store of this wave completes first.
__device__ __forceinline__ void hbm_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); }
template <class T>
__device__ __forceinline__ T ld_sc1(const T KS_G* p) {  // L1-bypassing load of HBM state other lanes wrote
  return __hip_atomic_load((T*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t lds_and(LU32 p, uint32_t v) {  // ds_and_rtn_b32
  return __hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}
// Wave-wide inclusive scans (sum / max) over the 64 lanes: DPP row_shr within each 16-lane row, then the
// rows' totals carried across by readlane.
__device__ __forceinline__ int wscan_add(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  const int r0 = __builtin_amdgcn_readlane(v, 15), r1 = r0 + __builtin_amdgcn_readlane(v, 31);
  const int r2 = r1 + __builtin_amdgcn_readlane(v, 47), l = lane();
  return v + (l >= 48 ? r2 : l >= 32 ? r1 : l >= 16 ? r0 : 0);
}
__device__ __forceinline__ int wscan_max(int v) {  // values >= -1
  auto mx = [](int a, int b) { return a > b ? a : b; };
  v = mx(v, __builtin_amdgcn_update_dpp(-1, v, 0x111, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(-1, v, 0x112, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(-1, v, 0x114, 0xf, 0xf, false));
  v = mx(v, __builtin_amdgcn_update_dpp(-1, v, 0x118, 0xf, 0xf, false));
  const int r0 = __builtin_amdgcn_readlane(v, 15), r1 = mx(r0, __builtin_amdgcn_readlane(v, 31));
  const int r2 = mx(r1, __builtin_amdgcn_readlane(v, 47)), l = lane();
  return mx(v, l >= 48 ? r2 : l >= 32 ? r1 : l >= 16 ? r0 : -1);
}
// Wave-wide reductions to a uniform value: DPP row_shr steps leave each 16-lane row's total in its lane 15,
// four readlanes combine the rows (no LDS round trip, unlike a __shfl_xor butterfly: ds_bpermute per step).
// Every lane must be active; `fill` is the operation's identity.
template <int CTRL>
__device__ __forceinline__ int dpp32(int old, int v) { return __builtin_amdgcn_update_dpp(old, v, CTRL, 0xf, 0xf, false); }
template <int CTRL>
__device__ __forceinline__ int64_t dpp64(int64_t old, int64_t v) {
  const int lo = dpp32<CTRL>((int)old, (int)v), hi = dpp32<CTRL>((int)(old >> 32), (int)(v >> 32));
  return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo);
}
template <int CTRL> __device__ __forceinline__ int dppT(int old, int v) { return dpp32<CTRL>(old, v); }
template <int CTRL> __device__ __forceinline__ uint32_t dppT(uint32_t old, uint32_t v) { return (uint32_t)dpp32<CTRL>((int)old, (int)v); }
template <int CTRL> __device__ __forceinline__ int64_t dppT(int64_t old, int64_t v) { return dpp64<CTRL>(old, v); }
template <int CTRL> __device__ __forceinline__ uint64_t dppT(uint64_t old, uint64_t v) { return (uint64_t)dpp64<CTRL>((int64_t)old, (int64_t)v); }
__device__ __forceinline__ int rdlT(int x, int l) { return rdl(x, l); }
__device__ __forceinline__ uint32_t rdlT(uint32_t x, int l) { return (uint32_t)rdl((int)x, l); }
__device__ __forceinline__ int64_t rdlT(int64_t x, int l) { return rdl64(x, l); }
__device__ __forceinline__ uint64_t rdlT(uint64_t x, int l) { return (uint64_t)rdl64((int64_t)x, l); }
template <class T, class F>
__device__ __forceinline__ T wred(T v, T fill, F op) {
  v = op(v, dppT<0x111>(fill, v));  // row_shr:1
  v = op(v, dppT<0x112>(fill, v));  // row_shr:2
  v = op(v, dppT<0x114>(fill, v));  // row_shr:4
  v = op(v, dppT<0x118>(fill, v));  // row_shr:8
  return op(op(rdlT(v, 15), rdlT(v, 31)), op(rdlT(v, 47), rdlT(v, 63)));
}
template <class T> __device__ __forceinline__ T wred_min(T v, T fill) { return wred(v, fill, [](T a, T b) { return b < a ? b : a; }); }
template <class T> __device__ __forceinline__ T wred_max(T v, T fill) { return wred(v, fill, [](T a, T b) { return b > a ? b : a; }); }
template <class T> __device__ __forceinline__ T wred_add(T v) { return wred(v, (T)0, [](T a, T b) { return a + b; }); }
// How many more pods requesting `req` of a resource fit a node with `free` of it, capped at m:
// floor(free / req) from a float estimate (rq ~ 1 / req from v_rcp_f32; relative error ~1e-7, so the
// estimate is within one of the quotient below m + 2 for any m < 10^6) corrected exactly by int64 multiplies.
// free < 0 (INT64_MIN marks a node that never fits) takes none.  req is wave-uniform (its branches are
// scalar); the per-lane part is branch-free: the estimate is clamped before the conversion and
// the correction and the bounds are selects.  req == 1 (the pods resource) needs no division.
__device__ __forceinline__ float run_rcp(int64_t req) { return req > 0 ? __builtin_amdgcn_rcpf((float)req) : 0.f; }
__device__ __forceinline__ int run_cap(int64_t free, int64_t req, float rq, int m) {
  if (req == 0) return free >= 0 ? m : 0;
  if (req == 1) return free <= 0 ? 0 : (free < (int64_t)m ? (int)free : m);
  const float q = fminf((float)free * rq, (float)(m + 2));
  int qi = q > 0.f ? (int)q : 0;
  qi -= (int64_t)qi * req > free ? 1 : 0;
  qi += (int64_t)(qi + 1) * req <= free ? 1 : 0;
  qi = qi < m ? qi : m;
  return free >= req ? qi : 0;
}

// Contiguous HBM -> LDS copy by the wave with U loads in flight per lane before their stores (a prologue's
// table staging is otherwise a chain of dependent round trips, one per 64 elements).
template <int U, class T>
__device__ __forceinline__ void lds_copy(T KS_L* dst, const T KS_G* src, int n) {
  int i = lane();
  for (; i + (U - 1) * kWave < n; i += U * kWave) {
    T v[U];
#pragma unroll
    for (int u = 0; u < U; u++) v[u] = src[i + u * kWave];
#pragma unroll
    for (int u = 0; u < U; u++) dst[i + u * kWave] = v[u];
  }
  for (; i < n; i += kWave) dst[i] = src[i];
}

#ifdef KS_PHASE_STATS
#define PH_BEGIN(v) uint64_t v = __builtin_amdgcn_s_memtime()
#define PH_END(v, slot) cyc[slot] += __builtin_amdgcn_s_memtime() - v
#define PHS_END(v, slot) scyc[slot] += __builtin_amdgcn_s_memtime() - v  // sub-phases (Solver member)
#define SPHS_END(o, v, slot) o.scyc[slot] += __builtin_amdgcn_s_memtime() - v  // (from k_solve)
#define FPH_END(v, slot) fcyc[slot] += __builtin_amdgcn_s_memtime() - v  // fine phases (k_solve, CT_FINE)
#define XPH_END(v, slot) xcyc[slot] += __builtin_amdgcn_s_memtime() - v  // the step's sub-phases (Solver member, CT_STEP)
#define SXPH_END(o, v, slot) o.xcyc[slot] += __builtin_amdgcn_s_memtime() - v  // (from k_solve)
#define XPH_COUNT(slot) xcyc[slot] += 1
#define YPH_END(v, slot) ycyc[slot] += __builtin_amdgcn_s_memtime() - v  // SS_TPL_DERIVE / SS_LOG split (Solver member, CT_CYC_SPLIT)
#define SYPH_END(o, v, slot) o.ycyc[slot] += __builtin_amdgcn_s_memtime() - v  // (from k_solve)
#define ZPH_END(v, slot) zcyc[slot] += __builtin_amdgcn_s_memtime() - v  // inside cycSort / cycCross (Solver member, CT_CYC_RESORT)
#define SZPH_END(o, v, slot) o.zcyc[slot] += __builtin_amdgcn_s_memtime() - v  // (from k_solve)
#define PH_WAIT_LOADS() __builtin_amdgcn_s_waitcnt(0x0f70)  // vmcnt(0): a stamp after it has waited for the loads
#else
#define PH_BEGIN(v)
#define PH_END(v, slot)
#define PHS_END(v, slot)
#define SPHS_END(o, v, slot)
#define FPH_END(v, slot)
#define XPH_END(v, slot)
#define SXPH_END(o, v, slot)
#define XPH_COUNT(slot)
#define YPH_END(v, slot)
#define SYPH_END(o, v, slot)
#define ZPH_END(v, slot)
#define SZPH_END(o, v, slot)
#define PH_WAIT_LOADS()
#endif

// ------------------------------------------------------------------------------------------------
// Init: per-replica workspace state (copies of the resident initial state), one grid-stride pass.
// ------------------------------------------------------------------------------------------------
#if KS_TU == 0
__global__ void k_init(KsDev D, const KsWork* works, int nrep, const int32_t* qorder) {
  const KsDims d = D.d;
  const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t gsz = (int64_t)gridDim.x * blockDim.x;
  for (int r = 0; r < nrep; r++) {
    const KsWork W = works[r];
    for (int64_t i = gtid; i < (int64_t)d.N * d.R; i += gsz) W.n_req[i] = D.n_req0[i];
    for (int64_t i = gtid; i < (int64_t)d.N * d.RSW; i += gsz) W.n_rs[i] = D.n_rs0[i];
    for (int64_t i = gtid; i < d.N; i += gsz) W.n_hp[i] = D.n_hp0[i];
    if (d.volAny)
      for (int64_t i = gtid; i < (int64_t)d.N * d.VD; i += gsz) W.n_vc[i] = D.n_vc0[i];
    if (d.G) {
      for (int64_t i = gtid; i < d.tgCntWords; i += gsz) W.tg_cnt[i] = D.tg_cnt0[i];
      for (int64_t i = gtid; i < (int64_t)d.G * (d.Kcap + 1); i += gsz) W.tg_ccnt[i] = 0;
      for (int64_t i = gtid; i < d.G; i += gsz) W.tg_cpos[i] = 0;
      for (int64_t i = gtid; i < d.G; i += gsz) W.tg_act[i] = 0;
      for (int64_t i = gtid; i < (int64_t)d.P * d.GMW; i += gsz) W.log_hg[i] = 0;
    }
    for (int64_t i = gtid; i < d.P; i += gsz) {
      W.queue[i] = qorder[i];
      W.pod_state[i] = D.pod_state0[i];
      W.pod_status[i] = ST_PENDING;
      W.pod_fstate[i] = -1;
    }
    for (int64_t i = gtid; i < d.NU; i += gsz) W.last_len[i] = 0;
    for (int64_t i = gtid; i < CT_NCOUNTERS; i += gsz) W.counters[i] = 0;
  }
}

// KS_LOG_RUNS: the commit-log entries of the run records a LEAN Solve left (KsWork::run_log, Solver::log_run_record),
// written after it by the whole GPU: entry nlog + e of a record (nlog, qhead, k, c) is pod qorder[qhead + e] on claim
// c.  A record is only written while the queue is NewQueue's order, so the pods are read from that order itself
// (k_init's source): a push-back later in the Solve may reuse the ring slots W.queue held them in.  The record count
// is read here, not on the host; k_solve stored none of these entries, so the two kernels' writes are disjoint.
__global__ __launch_bounds__(256) void k_log_expand(const KsWork* works, int nrep, const int32_t* qorder, int P) {
  for (int rep = blockIdx.y; rep < nrep; rep += gridDim.y) {
    const KsWork W = works[rep];
    const int64_t n = W.counters[CT_RUN_RECS];
    const int nrec = n < 0 ? 0 : n > P ? P : (int)n;  // (at most P records: KsWork::run_log)
    for (int r = blockIdx.x; r < nrec; r += gridDim.x) {
      const int nlog = W.run_log[4 * r], qh = W.run_log[4 * r + 1], k = W.run_log[4 * r + 2], c = W.run_log[4 * r + 3];
      if (nlog < 0 || qh < 0 || qh >= P || k <= 0 || k > P - nlog) continue;  // (never: the entries lie inside [0, P))
      for (int e = threadIdx.x; e < k; e += blockDim.x) {
        int q = qh + e;
        q = q >= P ? q - P : q;
        W.log_pod[nlog + e] = qorder[q];
        W.log_tgt[nlog + e] = c;
      }
    }
  }
}

#endif  // KS_TU == 0

// ------------------------------------------------------------------------------------------------
// Solve
// ------------------------------------------------------------------------------------------------
template <bool INL> struct ClaimView;
template <> struct ClaimView<true> { LI32 tpl; LI64 req; LI64 max; LU32 rem; LI32 thr; LI32 cnt; };
template <> struct ClaimView<false> { GI32 tpl; GI64 req; GI64 max; GU32 rem; GI32 thr; GI32 cnt; };

// One queue entry per lane (the 64-pod window), read wave-uniformly with readlane.
template <int RT>
struct Window {
  int p, g, uid, s, flags, pf, st;
  int rl;  // LEAN, nothing pushed back yet: identical pods from this queue position to the end of their run
  uint64_t ll, tol0, tol1, toltpl, hpc, hpu, hpo;
  uint64_t tsel, tinv, town, trss;  // TOPO: word 0 of the pod's selecting / inverse / owned group sets, st_rss keys
  int64_t req[RT > 0 ? RT : kMaxR];
};

// RT > 0: resource count known at compile time (loops unrolled, requests in VGPRs).
// TL: the instance-type tables (Allocatable per template position, sorted Allocatable lists) are
// LDS-resident.  Compile-time, so the hot loops carry no HBM branch (a join of an LDS and an HBM
// path would wait on vmcnt, i.e. on every outstanding store).
// SIM: a consolidation simulation (helpers.go:73-127) over the shared cluster problem: pods are
// the simulation's local subset (W.pod_map), the candidates' nodes are masked out, and existing
// node state is copy-on-write (a node's HBM slot is initialised the first time a pod lands on it).
// Requirements.Add (requirements.go:118-125) of `in` into `out`, both in LDS: the rs_add of
// ks_reqset.h with each key's words spread over the lanes (headers are wave-uniform; one wave,
// so every lane's reads of a key precede lane 0's header stores).  Returns whether a key of
// `mask` changed (what rs_equal_keys against the old record would report).
// Every branch is wave-uniform (the key loop, the per-key case, the 64-word blocks); the per-lane work is
// branch-free -- a lane past the key's last word computes on a clamped index and stores nothing, `diff` is
// accumulated by select -- and every header and bound store is a wave-wide store of a uniform value (DESIGN §3:
// the AMDGPU backend of this toolchain miscompiled divergent per-lane updates in loops; round 2's out-of-line
// form of this function worked around that without removing the pattern).
__device__ __forceinline__ bool rs_add_wave(const DevLayout& L, LU32 out, LU32 in, uint64_t mask) {
  const uint64_t pi = rs_present(in), po = rs_present(out);
  uint64_t cm = rs_compl(out), hg = rs_hasgt(out), hl = rs_haslt(out);
  const uint64_t icm = rs_compl(in), ihg = rs_hasgt(in), ihl = rs_haslt(in);
  uint32_t diff = 0;
  for (uint64_t m = pi; m; m &= m - 1) {
    const int k = ctz64(m);
    const uint64_t one = 1ull << k;
    const KeyMeta km = L.keys[k];
    const bool watched = (mask & one) != 0;
    const int base = L.HDR + km.off;
    if (po & one) {
      const KeyIx x = key_ix_header(L, out, in, k);
      for (int i0 = 0; i0 < km.nw; i0 += kWave) {
        const int i = i0 + lane();
        const bool live = i < km.nw;
        const int ic = live ? i : i0;
        const uint32_t old = out[base + ic];
        const uint32_t nw = key_ix_word(L, out, in, k, ic, x);
        if (live) out[base + i] = nw;
        diff |= (live && watched && nw != old) ? 1u : 0u;
      }
      const bool keep = !x.dne && x.compl_;
      const uint64_t ncm = keep ? (cm | one) : (cm & ~one);
      const uint64_t nhg = (keep && x.hg) ? (hg | one) : (hg & ~one);
      const uint64_t nhl = (keep && x.hl) ? (hl | one) : (hl & ~one);
      diff |= (watched && (((ncm ^ cm) | (nhg ^ hg) | (nhl ^ hl)) & one) != 0) ? 1u : 0u;
      cm = ncm;
      hg = nhg;
      hl = nhl;
      if (km.bslot >= 0) {
        const int64_t ngt = keep && x.hg ? x.gt : 0, nlt = keep && x.hl ? x.lt : 0;
        diff |= (watched && (ngt != rs_gt(out, km.bslot) || nlt != rs_lt(out, km.bslot))) ? 1u : 0u;
        wsync();
        rs_set_gt(out, km.bslot, ngt);  // wave-wide store of uniform values (see commit_claim)
        rs_set_lt(out, km.bslot, nlt);
      }
    } else {  // rs_copy_key
      for (int i0 = 0; i0 < km.nw; i0 += kWave) {
        const int i = i0 + lane();
        const bool live = i < km.nw;
        const uint32_t v = in[base + (live ? i : i0)];
        if (live) out[base + i] = v;
      }
      diff |= watched ? 1u : 0u;  // the key appears
      cm = (cm & ~one) | (icm & one);
      hg = (hg & ~one) | (ihg & one);
      hl = (hl & ~one) | (ihl & one);
      if (km.bslot >= 0) {
        const int64_t g = rs_gt(in, km.bslot), l = rs_lt(in, km.bslot);
        wsync();
        rs_set_gt(out, km.bslot, g);  // wave-wide store of uniform values
        rs_set_lt(out, km.bslot, l);
      }
    }
  }
  wsync();
  wr64(out, 0, po | pi);  // wave-wide store of uniform values (see commit_claim)
  wr64(out, 2, cm);
  wr64(out, 4, hg);
  wr64(out, 6, hl);
  wsync();
  return wballot(diff != 0) != 0;
}

// Requirements.Intersects(IT, X) (requirements.go:241-258) on the keys `keys` of X, for word wc of template
// t's position bitset, from the host's per-(key, value) position tables (ks_host.cpp "feasibility tables"):
// per key, the positions whose IT lacks the key (only shared keys are checked), those holding a value X
// admits, and -- when X's operator is NotIn / DoesNotExist -- those whose IT says DoesNotExist (both
// negative).  Every lane of the wave calls it with the same X, t and keys (ballots over X's values).
// dnePass: pass the DoesNotExist positions unconditionally (k_feasibility's factorised rows: whether
// they pass depends on the operator of the whole record, which feas_masks tests per step).
template <class PX>
__device__ __forceinline__ uint32_t fk_intersects_word(const KsDev& D, const DevLayout& L, PX X, int t, int wc,
                                                       uint64_t keys, bool dnePass = false) {
  const uint32_t KS_G* F = D.fk_words;
  const KsDims& d = D.d;
  const int TW = d.TW;
  uint32_t ic = ~0u;
  for (uint64_t m = keys; m; m &= m - 1) {
    const int k = ctz64(m);
    const int base = D.fk_key_off[t * d.NK + k];
    const KeyMeta km = L.keys[k];
    uint32_t acc = F[base + wc];  // positions whose IT lacks the key
    const int op = rs_op(L, X, k);
    if (dnePass || op == OP_NOTIN || op == OP_DNE) acc |= F[base + TW + wc];
    if (!bit(rs_compl(X), k)) {  // X In: the positions holding one of its values
      for (int i = 0; i < km.nw; i++) {
        uint32_t x = X[L.HDR + km.off + i];
        while (x) {
          const int v = i * 32 + __builtin_ctz(x);
          x &= x - 1;
          acc |= F[base + (3 + v) * TW + wc];
        }
      }
    } else if (!bit(d.fkMulti, k)) {  // complement, one value per IT: In positions minus the values X excludes
      uint32_t sub = 0;
      for (int v0 = 0; v0 < km.nv; v0 += kWave) {
        uint64_t out = wballot(v0 + lane() < km.nv && !rs_member(L, X, k, v0 + lane()));
        for (; out; out &= out - 1) sub |= F[base + (3 + v0 + ctz64(out)) * TW + wc];
      }
      acc |= F[base + 2 * TW + wc] & ~sub;
    } else {  // complement over multi-valued ITs: the values X admits
      for (int v0 = 0; v0 < km.nv; v0 += kWave) {
        uint64_t in = wballot(v0 + lane() < km.nv && rs_member(L, X, k, v0 + lane()));
        for (; in; in &= in - 1) acc |= F[base + (3 + v0 + ctz64(in)) * TW + wc];
      }
    }
    ic &= acc;
  }
  return ic;
}

#if KS_TU == 0
// Requirements.Intersects(IT, X) for word wc, as fk_intersects_word, evaluated by a group of GW lanes (GW = 32:
// the two halves of the wave work on different rows, each with its own X, t and key set; the complement
// branches ballot over the group's lanes only).
template <int GW, class PX>
__device__ __forceinline__ uint32_t fk_intersects_word_g(const KsDev& D, const DevLayout& L, PX X, int t, int wc,
                                                         uint64_t keys) {
  const uint32_t KS_G* F = D.fk_words;
  const KsDims& d = D.d;
  const int TW = d.TW;
  const int sub = lane() & (GW - 1), sh = GW == 64 ? 0 : (lane() & 32);
  auto gballot = [&](bool p) -> uint64_t {
    const uint64_t b = wballot(p);
    return GW == 64 ? b : (uint64_t)(uint32_t)(b >> sh);
  };
  uint32_t ic = ~0u;
  for (uint64_t m = keys; m; m &= m - 1) {
    const int k = ctz64(m);
    const int base = D.fk_key_off[t * d.NK + k];
    const KeyMeta km = L.keys[k];
    uint32_t acc = F[base + wc] | F[base + TW + wc];  // lacks the key; DoesNotExist (passed, see feas_masks)
    if (!bit(rs_compl(X), k)) {  // X In: the positions holding one of its values
      for (int i = 0; i < km.nw; i++) {
        uint32_t x = X[L.HDR + km.off + i];
        while (x) {
          const int v = i * 32 + __builtin_ctz(x);
          x &= x - 1;
          acc |= F[base + (3 + v) * TW + wc];
        }
      }
    } else if (!bit(d.fkMulti, k)) {  // complement, one value per IT: In positions minus the values X excludes
      uint32_t sbt = 0;
      for (int v0 = 0; v0 < km.nv; v0 += GW) {
        uint64_t out = gballot(v0 + sub < km.nv && !rs_member(L, X, k, v0 + sub));
        for (; out; out &= out - 1) sbt |= F[base + (3 + v0 + ctz64(out)) * TW + wc];
      }
      acc |= F[base + 2 * TW + wc] & ~sbt;
    } else {  // complement over multi-valued ITs: the values X admits
      for (int v0 = 0; v0 < km.nv; v0 += GW) {
        uint64_t in = gballot(v0 + sub < km.nv && rs_member(L, X, k, v0 + sub));
        for (; in; in &= in - 1) acc |= F[base + (3 + v0 + ctz64(in)) * TW + wc];
      }
    }
    ic &= acc;
  }
  return ic;
}

// k_feasibility (north_star "feasibility matrix"): the static part of the pod x
// instance-type feasibility per (relaxation state, template) row, over the words of the template's position
// bitset.  Row = Tolerates(template taints) AND Intersects(IT, template) AND Intersects(IT, state) on the keys
// no instance type constrains with more than one value (nodeclaim.go:68-71,225-260; requirements.go:241-258).
// k_solve ANDs the row where it would otherwise re-evaluate those keys per step (feas_masks); it tests the
// template's taints before it reads a row (try_templates, claim_quick), so an intolerant row is all zero and
// costs no reads.  HBM-bound: reads the state's and template's records and the template's position tables,
// writes TW words per row.
// Persistent 256-lane blocks: the key table is staged once per block, and each wave walks rows with a
// grid stride.  A row of TW <= 32 words takes half a wave (two rows per wave step), so lanes are not idle
// for the narrow template lists (C3: TW = 25).
template <int GW>
__global__ __launch_bounds__(256) void k_feasibility(KsDev D) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
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
  constexpr int RPW = 64 / GW;  // rows per wave step
  const int rows = d.S * d.NTPL;
  const int wave = (int)(threadIdx.x >> 6), half = GW == 64 ? 0 : (lane() >> 5), sub = lane() & (GW - 1);
  const uint64_t km = d.itKeys & ~d.fkMulti;
  for (int r0 = (blockIdx.x * 4 + wave) * RPW; r0 < rows; r0 += gridDim.x * 4 * RPW) {
    const int row = r0 + half;
    const bool live = row < rows;
    const int rr = live ? row : rows - 1;
    const int s = rr / d.NTPL, t = rr - s * d.NTPL;
    uint32_t KS_G* out = D.st_fm + (int64_t)rr * d.TW;
    if (!((D.st_toltpl[s] >> t) & 1ull)) {  // the state does not tolerate the template's taints
      for (int w = sub; w < d.TW; w += GW)
        if (live) out[w] = 0;
      continue;
    }
    const uint32_t KS_G* X = D.st_rs + (int64_t)s * d.RSW;
    const uint32_t KS_G* T = D.tpl_rs + (int64_t)t * d.RSW;
    const uint64_t kx = rs_present(X) & km, kt = rs_present(T) & km;
    for (int w0 = 0; w0 < d.TW; w0 += GW) {
      const int w = w0 + sub;
      const int wc = w < d.TW ? w : d.TW - 1;
      const uint32_t v = fk_intersects_word_g<GW>(D, L, X, t, wc, kx) & fk_intersects_word_g<GW>(D, L, T, t, wc, kt);
      if (live && w < d.TW) out[w] = v;
    }
  }
}
// k_feasibility_nodes (north_star "feasibility matrix", the existing-node side): per relaxation state with
// label requirements and per existing node, Taints.Tolerates AND the strict Requirements.Compatible of
// ExistingNode.Add (existingnode.go:64-124; taints.go:38-50; requirements.go:163-174) on the node's
// initial labels.  Both inputs are static for the whole Solve / pass, so k_solve's node scan reads one
// bit instead of re-running Compatible per (pod, node) step -- until a commit narrows a node's own
// requirements (existingnode.go:118), after which that node is tested exactly again.
// One thread per (row, node): a block of 256 nodes of one row; lanes evaluate their node against the same
// state record (uniform key loop), a ballot packs 64 node bits, lanes 0 and 32 store one word each.
__global__ __launch_bounds__(256) void k_feasibility_nodes(KsDev D, int nbx) {
  const KsDims& d = D.d;
  __shared__ __attribute__((aligned(16))) uint32_t s_kraw[64 * sizeof(KeyMeta) / 4];
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
  const int row = blockIdx.x / nbx, bx = blockIdx.x - row * nbx;
  const int s = D.fn_state[row];
  const uint32_t KS_G* X = D.st_rs + (int64_t)s * d.RSW;
  const uint64_t t0 = D.st_tol[2 * s], t1 = D.st_tol[2 * s + 1];
  const int NWN = (d.N + 31) >> 5;
  const int n = bx * 256 + (int)threadIdx.x;  // a wave's 64 nodes start at a multiple of 64
  bool ok = false;
  if (n < d.N) {
    const uint64_t KS_G* tp = D.n_taint + 2 * (int64_t)n;
    ok = ((tp[0] & ~t0) | (tp[1] & ~t1)) == 0 && rs_compatible(L, D.n_rs0 + (int64_t)n * d.RSW, X, 0);
  }
  const uint64_t b = wballot(ok);
  const int w = (n - lane()) >> 5;  // this wave's first word
  uint32_t KS_G* out = D.st_fn + (int64_t)row * NWN;
  if (lane() == 0 && w < NWN) out[w] = (uint32_t)b;
  if (lane() == 32 && w + 1 < NWN) out[w + 1] = (uint32_t)(b >> 32);
}
#endif

// A topology simulation keeps its register window's node domains in LDS (Solver::s_tdw): the first kTdw nodes,
// the first kTdwKeys key slots (make_plan counts the bytes).
constexpr int kTdw = 256, kTdwKeys = 4;

// The claim order and its re-sort: s.newNodeClaims as claim ids and pod counts per sorted position, and the
// wave-parallel replay of Go's pdqsort_func over them.  Kept apart from Solver (which derives from it) so that the
// general re-sort can run out of line on the two LDS arrays alone (claim_sort_general).
struct ClaimSort {
  LI32 s_order;         // [KO] s.newNodeClaims as claim ids
  LI32 s_okey;          // [KO] len(Pods) of the claim at each position
#ifdef KS_PHASE_STATS
  uint64_t pivcyc = 0;  // cycles of w_choose_pivot inside closed_crossing (added to cycPivot)
#endif
  // --- s.newNodeClaims re-sort (scheduler.go:247) --------------------------------------------------
  // Called only when the array is not non-decreasing (a non-decreasing array is provably left
  // untouched by pdqsort).  Lane 0 replays Go's pdqsort_func; the position-indexed quick-reject
  // arrays are then regathered from the claims.
  // Move the entry at position `from` to `to`, shifting the ones between by one (wave-parallel, in
  // 64-entry chunks ordered so every chunk is read before it is overwritten).  Equals the adjacent
  // swap chains of partialInsertionSort.
  __device__ __forceinline__ void pis_move(int from, int to) {
    if (from == to) return;
    const int k0 = uni(s_okey[from]), v0 = uni(s_order[from]);
    wsync();
    if (to < from) {  // [to, from) shifts right, high chunk first
      for (int hi = from; hi > to; hi -= kWave) {
        const int lo = hi - kWave > to ? hi - kWave : to, j = lo + lane();
        int k = 0, v = 0;
        if (j < hi) { k = s_okey[j]; v = s_order[j]; }
        wsync();
        if (j < hi) { s_okey[j + 1] = k; s_order[j + 1] = v; }
        wsync();
      }
    } else {  // (from, to] shifts left, low chunk first
      for (int lo = from + 1; lo <= to; lo += kWave) {
        const int hi = lo + kWave <= to + 1 ? lo + kWave : to + 1, j = lo + lane();
        int k = 0, v = 0;
        if (j < hi) { k = s_okey[j]; v = s_order[j]; }
        wsync();
        if (j < hi) { s_okey[j - 1] = k; s_order[j - 1] = v; }
        wsync();
      }
    }
    s_okey[to] = k0;  // wave-wide store of uniform values (see commit_claim)
    s_order[to] = v0;
    wsync();
  }
  // First i in [from, n) with key[i] < key[i-1] (a descent), or n.  Four chunks per round trip: the
  // scan usually runs to the end of the array (proving it sorted), so it is latency-bound.
  __device__ __forceinline__ int pis_descent(int from, int n) const {
    for (int base = from; base < n; base += 4 * kWave) {
      uint64_t m[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = base + u * kWave + lane();
        const int k1 = i < n ? s_okey[i] : 0, k0 = i < n ? s_okey[i - 1] : 0;
        m[u] = wballot(k1 < k0);
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (m[u]) return base + u * kWave + ctz64(m[u]);
    }
    return n;
  }
  // (the medians below are also choose_pivot_medians of ks_sort_regs.h, the register copy's: a change here is a
  // change there; sharing one form changed the code of every k_solve instantiation)
  // choosePivot_func (zsortfunc.go): the wave reads the (up to) nine samples at once, lane t sample t,
  // and the medians run on scalars; same pivot and hint as GoSortT::choosePivot.
  __device__ __forceinline__ int w_choose_pivot(int a, int b, int& hint) const {
    return w_choose_pivot_at(a, b, hint, [this](int pos) { return s_okey[pos]; });
  }
  // ... on the array a run's deferred move stands for (KS_RUN_FUSE): the claim taken from pos0 and put at p with
  // key K, the entries between one place to the left -- index i in [pos0, p) reads i + 1, p reads K
  __device__ __forceinline__ int w_choose_pivot_moved(int n, int pos0, int p, int K, int& hint) const {
    return w_choose_pivot_at(0, n, hint, [this, pos0, p, K](int pos) {
      const int k = s_okey[pos >= pos0 && pos < p ? pos + 1 : pos];
      return pos == p ? K : k;
    });
  }
  template <class F>
  __device__ __forceinline__ int w_choose_pivot_at(int a, int b, int& hint, F keyAt) const {
    const int l = b - a;
    int i = a + l / 4, j = a + l / 4 * 2, k = a + l / 4 * 3, swaps = 0;
    if (l >= 8) {
      const int t = lane() < 9 ? lane() : 0, g = t / 3;
      const int pos = (g == 0 ? i : g == 1 ? j : k) + (t % 3) - 1;
      const int key = keyAt(pos);
      int ik[9], kk[9];
#pragma unroll
      for (int u = 0; u < 9; u++) {
        ik[u] = (u / 3 == 0 ? i : u / 3 == 1 ? j : k) + (u % 3) - 1;
        kk[u] = rdl(key, u);
      }
      auto median = [&](int ia, int ka, int ib, int kb, int ic, int kc, int& km) {
        if (kb < ka) { swaps++; int t0 = ia; ia = ib; ib = t0; t0 = ka; ka = kb; kb = t0; }
        if (kc < kb) { swaps++; int t0 = ib; ib = ic; ic = t0; t0 = kb; kb = kc; kc = t0; }
        if (kb < ka) { swaps++; int t0 = ia; ia = ib; ib = t0; t0 = ka; ka = kb; kb = t0; }
        km = kb;
        return ib;
      };
      int ki = kk[1], kj = kk[4], kq = kk[7];
      if (l >= 50) {
        i = median(ik[0], kk[0], ik[1], kk[1], ik[2], kk[2], ki);
        j = median(ik[3], kk[3], ik[4], kk[4], ik[5], kk[5], kj);
        k = median(ik[6], kk[6], ik[7], kk[7], ik[8], kk[8], kq);
      }
      int km = 0;
      j = median(i, ki, j, kj, k, kq, km);
    }
    hint = swaps == 0 ? 1 : (swaps == 12 ? 2 : 0);
    return j;
  }
  // KS_PIVOT_ARITH: is `pos` or pos + 1 inside one of choosePivot's three sample triples of [0, n), n >= 50?  The
  // triples are {l-1, l, l+1}, {2l-1, 2l, 2l+1}, {3l-1, 3l, 3l+1}, l = n/4 >= 12: a descent between pos and pos + 1
  // is seen by a median network exactly when both lie in one triple.  On an array non-decreasing but for that
  // descent, every other comparison of choosePivot finds its pair in order (the three medians are then the middle
  // samples l, 2l, 3l, whose keys the increment did not lift above a later sample's): no swap, hint "increasing",
  // pivot 2l.
  static __device__ __forceinline__ bool pivot_sampled(int n, int pos) {
    const int l = n / 4, e = pos - (l - 1);
    return e == 0 || e == 1 || e == l || e == l + 1 || e == 2 * l || e == 2 * l + 1;
  }
  // partialInsertionSort_func(data, 0, n) of Go 1.21 (zsortfunc.go), wave-parallel: each of its <= 5
  // steps finds the next descent by ballot, swaps the pair, then moves the smaller entry left past
  // every greater one and the greater entry right past every smaller one.  Returns its result and
  // widens [tlo, thi] to the positions it moved.
  __device__ __forceinline__ bool pis_wave(int a, int b, int& tlo, int& thi) {
    int i = a + 1;
    for (int step = 0; step < 5; step++) {
      i = pis_descent(i, b);
      if (i == b) return true;
      if (b - a < 50) return false;
      const int x = uni(s_okey[i]), y = uni(s_okey[i - 1]);  // after the swap: x at i-1, y at i
      int p = i - 1;  // x passes the entries q < i-1 with x < key[q] (Go's loop runs down to index 1,
      if (i - a >= 2) {  // not to a, once the pair is at least two past a)
        for (int hi = i - 1; hi > 0; hi -= kWave) {
          const int q = hi - 1 - lane();
          const uint64_t m = wballot(q >= 0 && !(x < s_okey[q]));
          if (m) { p = hi - ctz64(m); break; }
          p = hi - kWave > 0 ? hi - kWave : 0;
        }
      }
      int r = i;  // y passes the entries q > i with key[q] < y
      for (int lo = i + 1; lo < b; lo += kWave) {
        const int q = lo + lane();
        const uint64_t m = wballot(q < b && !(s_okey[q] < y));
        if (m) { r = lo + ctz64(m) - 1; break; }
        r = lo + kWave - 1 < b - 1 ? lo + kWave - 1 : b - 1;
      }
      pis_move(i, p);  // x (at i before the swap) to p; y moves from i-1 to i with the shifted run
      pis_move(i, r);  // y to r
      tlo = p < tlo ? p : tlo;
      thi = r > thi ? r : thi;
    }
    return false;
  }

  // --- the rest of pdqsort_func, wave-parallel and swap-for-swap equal to Go's (ks_gosort.h) -------
  // Exchange of two uniform positions (wave-wide stores of uniform values).
  __device__ __forceinline__ void w_swap(int i, int j) {
    const int ki = uni(s_okey[i]), kj = uni(s_okey[j]), vi = uni(s_order[i]), vj = uni(s_order[j]);
    wsync();
    s_okey[i] = kj;
    s_order[i] = vj;
    wsync();
    s_okey[j] = ki;
    s_order[j] = vi;
    wsync();
  }
  // Entries of [a, b) whose key is below `pk` (below_or_eq: at most `pk`).
  __device__ __forceinline__ int w_count(int a, int b, int pk, bool below_or_eq) const {
    int c = 0;
    for (int base = a; base < b; base += kWave) {
      const int p = base + lane();
      const int k = p < b ? s_okey[p] : 0;
      c += __popcll(wballot(p < b && (below_or_eq ? k <= pk : k < pk)));
    }
    return c;
  }
  // A Hoare pass (partition_func / partitionEqual_func) whose boundary `m` is known up front: its i scan
  // stops on the left region's entries [l0, m) of the wrong side, its j scan on the right region's
  // [m, r1), and it exchanges the k-th from the left with the k-th from the right, for every k (the two
  // counts are equal, and the scans cross exactly at the boundary).  `eq` selects partitionEqual's
  // predicates (wrong on the left: key > pk) over partition's (key >= pk).  Returns the exchange count.
  __device__ int w_hoare(int l0, int m, int r1, int pk, bool eq) {
    int lb = l0, rb = r1, lbase = 0, rtop = 0, swaps = 0;
    uint64_t mL = 0, mR = 0;
    for (;;) {
      if (mL == 0) {
        if (lb >= m) break;
        const int p = lb + lane();
        const int k = p < m ? s_okey[p] : 0;
        mL = wballot(p < m && (eq ? k > pk : k >= pk));
        lbase = lb;
        lb += kWave;
        continue;
      }
      if (mR == 0) {
        if (rb <= m) break;
        const int p = rb - 1 - lane();  // bit t <-> position rtop - t: ascending bits walk down from r1
        const int k = p >= m ? s_okey[p] : 0;
        mR = wballot(p >= m && (eq ? k <= pk : k < pk));
        rtop = rb - 1;
        rb -= kWave;
        continue;
      }
      const int nL = __popcll(mL), nR = __popcll(mR), np = nL < nR ? nL : nR;
      const uint64_t below = (1ull << lane()) - 1ull;
      const bool inL = (mL >> lane()) & 1ull, inR = (mR >> lane()) & 1ull;
      const int rkL = __popcll(mL & below), rkR = __popcll(mR & below);
      // ds_permute pushes every lane's position to its rank (a bijection over the 64 lanes)
      const int dL = inL ? rkL : nL + (lane() - rkL), dR = inR ? rkR : nR + (lane() - rkR);
      const int posL = __builtin_amdgcn_ds_permute(dL * 4, lbase + lane());
      const int posR = __builtin_amdgcn_ds_permute(dR * 4, rtop - lane());
      if (lane() < np) {  // disjoint positions: the lanes' exchanges do not overlap
        const int kl = s_okey[posL], vl = s_order[posL], kr = s_okey[posR], vr = s_order[posR];
        s_okey[posL] = kr;
        s_order[posL] = vr;
        s_okey[posR] = kl;
        s_order[posR] = vl;
      }
      wsync();
      for (int t = 0; t < np; t++) {
        mL &= mL - 1;
        mR &= mR - 1;
      }
      swaps += np;
    }
    return swaps;
  }
  // partition_func: returns the new pivot position; `already` = no exchange was needed.
  __device__ __forceinline__ int w_partition(int a, int b, int pivot, bool& already) {
    w_swap(a, pivot);
    const int pk = uni(s_okey[a]);
    const int j = a + w_count(a + 1, b, pk, false);
    already = w_hoare(a + 1, j + 1, b, pk, false) == 0;
    w_swap(j, a);
    return j;
  }
  // partitionEqual_func: returns the first position past the entries equal to the pivot.
  __device__ __forceinline__ int w_partition_equal(int a, int b, int pivot) {
    w_swap(a, pivot);
    const int pk = uni(s_okey[a]);
    const int m = a + 1 + w_count(a + 1, b, pk, true);
    w_hoare(a + 1, m, b, pk, true);
    return m;
  }
  __device__ __forceinline__ void w_reverse(int a, int b) {
    const int h = (b - a) / 2;
    for (int base = 0; base < h; base += kWave) {
      const int t = base + lane();
      if (t < h) {
        const int i = a + t, j = b - 1 - t;
        const int ki = s_okey[i], vi = s_order[i], kj = s_okey[j], vj = s_order[j];
        s_okey[i] = kj;
        s_order[i] = vj;
        s_okey[j] = ki;
        s_order[j] = vi;
      }
    }
    wsync();
  }
  // insertionSort_func on [a, b), b - a <= 12 (KS_SORT_LEAF): it exchanges only a strictly smaller entry with its
  // left neighbour, so it is a stable sort and its result is the stable-rank permutation.  Lane i holds entry
  // a + i, reads the others' keys by readlane, counts the entries that sort before its own and stores to its rank:
  // one LDS read, one write (tests/test_sort_leaf_model.py).
  __device__ __forceinline__ void w_leaf(int a, int b) {
    const int len = b - a, l = lane();
    if (len < 2) return;
    const bool me = l < len;
    const int mk = me ? s_okey[a + l] : 0, mv = me ? s_order[a + l] : 0;
    int rank = 0;
#pragma unroll 1  // (unrolled, its twelve scalars cost the out-of-line re-sort a callee-saved register: a scratch slot)
    for (int j = 0; j < len; j++) {
      const int kj = rdl(mk, j);
      rank += kj < mk || (kj == mk && j < l) ? 1 : 0;
    }
    wsync();
    if (me) {  // rank < len: a permutation of [a, b)
      s_okey[a + rank] = mk;
      s_order[a + rank] = mv;
    }
    wsync();
  }
  // The closed form of a re-sort whose choosePivot gave the increasing hint, n >= 50, 0 <= pos < n - 1:
  // the descent is the one a count increment at `pos` left: non-decreasing but key[pos] > key[pos+1].
  // partialInsertionSort then swaps the pair, finds nothing to move left (key[pos+1] >= key[pos] - 1 >=
  // key[pos-1]), walks the claim right past the t entries below its key and meets no second descent:
  // (pos, pos+t] moves one place left, the claim lands at pos + t (tests/test_sort_single_descent.py).
  // The entries past pos are sorted, so those below the key are the first t of them.
  // Moves s_okey and s_order and returns t; -1 (nothing moved) when there is no descent at pos.
  __device__ __forceinline__ int closed_move(int n, int pos) {
    const int K = uni(s_okey[pos]);
    if (!(K > uni(s_okey[pos + 1]))) return -1;
    int t = 0;
    for (int base = pos + 1; base < n; base += 4 * kWave) {  // four chunks per round trip (pis_descent)
      uint64_t m[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int q = base + u * kWave + lane();
        m[u] = wballot(q < n && s_okey[q] < K);
      }
      bool end = false;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        t += end ? 0 : popc64(m[u]);
        end = end || m[u] != ~0ull;
      }
      if (end) break;
    }
    pis_move(pos, pos + t);
    return t;
  }
  // The top-level frame of a re-sort of n > 12 entries after a count increment at `pos` (-1: another origin), with
  // the closed form's move done on all four position arrays (KS_CLOSED_SHIFT).  choosePivot as w_choose_pivot
  // (`pv`, `hint`); when it gives the increasing hint and the single descent is the one the increment left
  // (sort_claims), the t entries below the claim's key K -- the first t past pos, the rest being sorted -- move
  // one place left in s_okey, s_order, ptpl and phead ([.][R]) and the claim's own entries go to pos + t.  Returns
  // t, or -1 with the arrays untouched.
  // The reads that do not depend on each other are issued together: the nine samples, K, the next key and the first
  // 256 keys past pos; then the moved entries of the four arrays, 256 positions per read and write batch, low
  // positions first (a batch writes one place below what it read: below itself, or onto pos, read before).
  // PA (KS_PIVOT_ARITH): with the descent at pos confirmed and pos off the sample triples the hint and the pivot are
  // arithmetic (`arith`) and the nine samples are not read: the batch is K, the next key and the 256 keys.
  template <int R, bool PA>
  __device__ __forceinline__ int closed_crossing(int n, int pos, LI32 ptpl, LI64 phead, int& hint, int& pv, bool& arith) {
    const bool cand = pos >= 0 && n >= 50 && pos + 1 < n;
    const int pc = cand ? pos : 0;  // (n > 12: the reads stay inside the array for any pos)
    const int K = s_okey[pc], nx = s_okey[pc + 1];
    int kq[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      // (an unconditional read of a clamped position: a read under `q < n` becomes a branch with its own wait)
      const int q = pc + 1 + u * kWave + lane(), k = s_okey[q < n ? q : n - 1];
      kq[u] = q < n ? k : INT32_MAX;
    }
    arith = false;
    if constexpr (PA) arith = cand && !pivot_sampled(n, pc) && ub(K > nx);
    if (arith) {
      hint = 1;
      pv = n / 4 * 2;
    } else {
#ifdef KS_PHASE_STATS
      const uint64_t tpv = __builtin_amdgcn_s_memtime();
#endif
      pv = w_choose_pivot(0, n, hint);
#ifdef KS_PHASE_STATS
      pivcyc += __builtin_amdgcn_s_memtime() - tpv;  // (the stamp also waits for the key batch issued above)
#endif
      if (!cand || hint != 1 || !ub(K > nx)) return -1;
    }
    int t = 0;
    bool end = false;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const uint64_t m = wballot(kq[u] < K);
      t += end ? 0 : popc64(m);
      end = end || m != ~0ull;
    }
    for (int base = pos + 1 + 4 * kWave; !end && base < n; base += 4 * kWave) {
      uint64_t m[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int q = base + u * kWave + lane();
        m[u] = wballot(q < n && s_okey[q] < K);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        t += end ? 0 : popc64(m[u]);
        end = end || m[u] != ~0ull;
      }
    }
    const int to = pos + t;  // <= n - 1
    const int v0 = s_order[pos], tp0 = ptpl[pos];  // uniform addresses: every lane holds the claim's entries
    int64_t h0[R];
#pragma unroll
    for (int r = 0; r < R; r++) h0[r] = phead[(int64_t)pos * R + r];
    for (int lo = pos + 1; lo <= to; lo += 4 * kWave) {
      int k[4], v[4], tp[4];
      int64_t h[4][R];
      const int nu = (to - lo) / kWave + 1;  // chunks of this batch that hold moved entries (uniform)
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (u < nu) {  // (reads of clamped positions, as above)
          const int j = lo + u * kWave + lane(), jj = j <= to ? j : to;
          k[u] = s_okey[jj];
          v[u] = s_order[jj];
          tp[u] = ptpl[jj];
#pragma unroll
          for (int r = 0; r < R; r++) h[u][r] = phead[(int64_t)jj * R + r];
        }
      }
      wsync();
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int j = lo + u * kWave + lane();
        if (u < nu && j <= to) {
          s_okey[j - 1] = k[u];
          s_order[j - 1] = v[u];
          ptpl[j - 1] = tp[u];
#pragma unroll
          for (int r = 0; r < R; r++) phead[(int64_t)(j - 1) * R + r] = h[u][r];
        }
      }
      wsync();
    }
    s_okey[to] = K;  // wave-wide stores of uniform values (see commit_claim)
    s_order[to] = v0;
    ptpl[to] = tp0;
#pragma unroll
    for (int r = 0; r < R; r++) phead[(int64_t)to * R + r] = h0[r];
    wsync();
    return t;
  }
  // The closed form of a re-sort after an appended claim (KS_APPEND_CLOSED), n >= 50: non-decreasing on [0, n-1),
  // key[n-1] < key[n-2].  choosePivot's samples end at 3(n/4) + 1 < n - 1 and find the array increasing;
  // partialInsertionSort swaps the last pair, walks the new entry left past every greater key and meets no second
  // descent (tests/test_pivot_arith_model.py).  With p = #{q < n-1 : key[q] <= key[n-1]}, the first p entries of a
  // sorted prefix, [p, n-1) moves one place right in s_okey, s_order, ptpl and phead ([.][R]), high chunk first and
  // each chunk read before it is written, and the new claim's entries go to p.  Returns p, or -1 with the arrays
  // untouched when the last entry is not below its neighbour.
  template <int R>
  __device__ __forceinline__ int append_closed(int n, LI32 ptpl, LI64 phead) {
    const int K = s_okey[n - 1], pk = s_okey[n - 2];  // uniform addresses: every lane holds the new claim's entries
    const int v0 = s_order[n - 1], tp0 = ptpl[n - 1];
    int64_t h0[R];
#pragma unroll
    for (int r = 0; r < R; r++) h0[r] = phead[(int64_t)(n - 1) * R + r];
    if (!ub(K < pk)) return -1;
    int p = 0;
    for (int base = 0; base < n - 1; base += kWave) {
      const int q = base + lane();
      const uint64_t m = wballot(q < n - 1 && s_okey[q] <= K);
      p += popc64(m);
      if (m != ~0ull) break;
    }
    wsync();
    for (int hi = n - 1; hi > p; hi -= kWave) {
      const int lo = hi - kWave > p ? hi - kWave : p, j = lo + lane();
      int k = 0, v = 0, tp = 0;
      int64_t h[R];
      if (j < hi) {
        k = s_okey[j];
        v = s_order[j];
        tp = ptpl[j];
#pragma unroll
        for (int r = 0; r < R; r++) h[r] = phead[(int64_t)j * R + r];
      }
      wsync();
      if (j < hi) {
        s_okey[j + 1] = k;
        s_order[j + 1] = v;
        ptpl[j + 1] = tp;
#pragma unroll
        for (int r = 0; r < R; r++) phead[(int64_t)(j + 1) * R + r] = h[r];
      }
      wsync();
    }
    s_okey[p] = K;  // wave-wide stores of uniform values (see commit_claim)
    s_order[p] = v0;
    ptpl[p] = tp0;
#pragma unroll
    for (int r = 0; r < R; r++) phead[(int64_t)p * R + r] = h0[r];
    wsync();
    return p;
  }
  // GoSortExactT::run with the whole wave: frames live one per lane (lane k = stack slot k), the
  // partitions, reversals and partialInsertionSorts run wave-parallel, and so do the frames of <= 12 entries
  // (w_leaf); heapSort (the depth limit) and breakPatterns stay on lane 0.  resumePivot as in run().
  // LEAF: w_leaf for the frames of <= 12 entries (the LEAN Solve: in the other instantiations, whose re-sort is
  // inlined, it measured slower on C4 and C5 + topology)
  template <bool LEAF>
  __device__ void w_pdqsort(int n, int resumePivot) {
    int fa = 0, fb = 0, fl = 0, ff = 0;  // this lane's stack slot: a, b, limit, flags (wb | wp << 1)
    int sp = 0;
    {
      const bool me = lane() == 0;
      fa = me ? 0 : fa;
      fb = me ? n : fb;
      fl = me ? GoSortT<LI32>::bitsLen((uint32_t)n) : fl;
      ff = me ? 3 : ff;
      sp = 1;
    }
    bool resume = resumePivot >= 0;
    int dummy_lo = 0, dummy_hi = 0;
    while (sp > 0) {
      sp--;
      int a = rdl(fa, sp), b = rdl(fb, sp), limit = rdl(fl, sp);
      const int flags = rdl(ff, sp);
      bool wasBalanced = flags & 1, wasPartitioned = (flags >> 1) & 1;
      for (;;) {
        const int length = b - a;
        int pivot;
        if (resume) {
          resume = false;
          pivot = resumePivot;
        } else {
          if (KS_SORT_LEAF && LEAF && length <= 12) {
            w_leaf(a, b);
            break;
          }
          if (length <= 12 || limit == 0) {
            if (lane() == 0) {
              GoSortT<LI32> g{s_okey, s_order};
              if (length <= 12) g.insertionSort(a, b);
              else g.heapSort(a, b);
            }
            wsync();
            break;
          }
          if (!wasBalanced) {
            if (lane() == 0) {
              GoSortT<LI32> g{s_okey, s_order};
              g.breakPatterns(a, b);
            }
            wsync();
            limit--;
          }
          int hint = 0;
          pivot = w_choose_pivot(a, b, hint);
          if (hint == 2) {
            w_reverse(a, b);
            pivot = (b - 1) - (pivot - a);
            hint = 1;
          }
          if (wasBalanced && wasPartitioned && hint == 1 && pis_wave(a, b, dummy_lo, dummy_hi)) break;
        }
        if (a > 0 && ub(!(s_okey[a - 1] < s_okey[pivot]))) {
          a = w_partition_equal(a, b, pivot);
          continue;
        }
        bool already = false;
        const int mid = w_partition(a, b, pivot, already);
        wasPartitioned = already;
        const int leftLen = mid - a, rightLen = b - mid, thr = length / 8;
        if (sp + 2 > kWave) return;  // unreachable: depth <= 2*log2(n) + 2
        int c0a, c0b, c1a, c1b;
        if (leftLen < rightLen) {
          wasBalanced = leftLen >= thr;
          c0a = mid + 1; c0b = b; c1a = a; c1b = mid;  // continuation, then the recursive call
        } else {
          wasBalanced = rightLen >= thr;
          c0a = a; c0b = mid; c1a = mid + 1; c1b = b;
        }
        const bool m0 = lane() == sp, m1 = lane() == sp + 1;
        fa = m0 ? c0a : (m1 ? c1a : fa);
        fb = m0 ? c0b : (m1 ? c1b : fb);
        fl = (m0 || m1) ? limit : fl;
        ff = m0 ? ((int)wasBalanced | ((int)wasPartitioned << 1)) : (m1 ? 3 : ff);
        sp += 2;
        break;
      }
    }
  }
};
// The wave's operations for SortRegsT (ks_sort_regs.h)
struct SortRegsWaveOps {
  using Vec = int;
  template <class F> static __device__ __forceinline__ void each(F f) { f(lane()); }
  static __device__ __forceinline__ int& at(Vec& v, int) { return v; }
  static __device__ __forceinline__ int get(const Vec& v, int) { return v; }
  static __device__ __forceinline__ int rdl(Vec v, int l) { return __builtin_amdgcn_readlane(v, l); }
  template <class F> static __device__ __forceinline__ uint64_t ballot(F p) { return wballot(p(lane())); }
  template <class F> static __device__ __forceinline__ Vec gather(Vec v, F src) {
    return __builtin_amdgcn_ds_bpermute(src(lane()) * 4, v);
  }
  template <class F> static __device__ __forceinline__ Vec scatter(Vec v, F dst) {
    return __builtin_amdgcn_ds_permute(dst(lane()) * 4, v);
  }
};
// The general re-sort: partialInsertionSort when choosePivot gave the increasing hint (pivot >= 0), else or after
// it the exact pdqsort.  claim_sort_general_out is the same out of line (KS_SORT_OUTLINE), so a kernel holds one copy
// for its two call sites; the arguments are the two LDS arrays, not the Solver (a pointer to which would force its
// state into memory).
// Returns tlo | (thi + 1) << 15 | done << 30 (positions < 2^14: KsDims::Kcap).
// REGS (KS_SORT_REGS; the LEAN Solve's out-of-line copy and the probe): up to kSortRegsMax entries are sorted on a
// register copy, stored once, and the word carries kSortRegsDone; after a bail-out the arrays are as they were and
// the LDS code below sorts them.
template <bool LEAF, bool REGS = false>
static __device__ __forceinline__ uint32_t claim_sort_general(LI32 okey, LI32 order, int n, int pivot) {
  if constexpr (REGS && KS_SORT_REGS != 0) {
    n = uni(n);
    pivot = uni(pivot);
    if (n <= (KS_SORT_REGS_N64 ? 64 : kSortRegsMax)) {
      SortRegsT<SortRegsWaveOps, !KS_SORT_REGS_N64> rs;
      rs.load(n, [&](int p) { return okey[p]; }, [&](int p) { return order[p]; });
      const uint32_t g = rs.general(pivot);
      if (g != 0) {
        rs.store([&](int p, int k, int v) {
          okey[p] = k;
          order[p] = v;
        });
        wsync();
        return g;
      }
    }
  }
  ClaimSort cs;
  cs.s_order = order;
  cs.s_okey = okey;
  int tlo = n, thi = -1;
  bool done = false;
  if (pivot >= 0) done = cs.pis_wave(0, n, tlo, thi);
  if (!done) {
#if KS_SORT_LANE0
    if (lane() == 0) {
      GoSortExactT<LI32> g{GoSortT<LI32>{okey, order}};
      g.run(n, pivot);
    }
#else
    cs.template w_pdqsort<LEAF>(n, pivot);
#endif
    tlo = 0;
    thi = n - 1;
  }
  return (uint32_t)tlo | (uint32_t)(thi + 1) << 15 | (uint32_t)done << 30;
}
static __device__ __noinline__ uint32_t claim_sort_general_out(LI32 okey, LI32 order, int n, int pivot) {
  return claim_sort_general<true, true>(okey, order, n, pivot);
}

template <int RT, bool TL, bool SIM, bool TOPO, bool LEAN, bool SLOG = false>
struct Solver : ClaimSort {
  static constexpr int RM = RT > 0 ? RT : kMaxR;
  // LEAN: the problem uses none of host ports, limited volumes, pod label requirements, shared UIDs,
  // negative requests or topology (KsDims::lean, set by the encoder).  Those paths compile out, which
  // frees the registers they pinned (SGPR spills) and the instructions they cost on every pop.
  static_assert(!(LEAN && TOPO), "LEAN excludes topology");
  __device__ __forceinline__ bool hpA() const { return !LEAN && d.hpAny; }
  __device__ __forceinline__ bool volA() const { return !LEAN && d.volAny; }
  __device__ __forceinline__ bool negR() const { return !LEAN && d.negReq; }
  __device__ __forceinline__ bool dupU() const { return !LEAN && d.dupUids; }
  __device__ __forceinline__ bool keys(int sflags) const { return !LEAN && (sflags & SF_HAS_KEYS); }
  // By value: a reference to a byval kernel argument forces a scratch copy of the whole struct
  // (every field access then becomes a scratch load); values scalarise into SGPRs.
  // Launch constants by reference, not by copy: the kernel arguments stay in the kernarg segment and
  // the work descriptor in constant memory, read with scalar loads where used.  (Copies of these
  // ~1 KB structs did not fit the SGPRs and lived in scratch memory: a private-memory round trip
  // on many hot-path reads.)
  const KsDev& D;
  const KsDims& d;
  const KsWork KS_C& W;
  const Plan& pl;
  DevLayout L;
  ClaimView<true> lc;   // claims [0, KL)
  ClaimView<false> gc;  // claims [KL, KO)
  LI32 s_ptpl;          // [KO] template of the claim at each position
  LI64 s_phead;         // [KO][R] max Allocatable - requests of the claim at each position
  LI64 s_talloc;        // [totalTplIts][R] Allocatable per template position (pl.talloc)
  LI64 s_tsa;           // tsort_alloc (pl.tsort)
  LI32 s_tsp;           // tsort_pos (pl.tsort)
  LI32 s_tbeg;          // [NTPL+1]
  LI64 s_pool;          // [NPOOL][R] remaining limits
  LU32 s_rs;            // [RSW] candidate requirements
  LU32 s_pin;           // [RSW] the popped pod's requirement record (its relaxation state), when it has keys
  LU32 s_rem;           // [TW+2] candidate options
  LU32 s_cand;          // [TW+2] limit-filtered template options
  LU32 s_fic;           // [TW+2] feas_masks: Intersects(IT, X) per position
  LU32 s_fof;           // [TW+2] feas_masks: hasOffering(IT, X) per position
  LU32 s_firr;          // [TW+2] feas_masks: irregular positions (exact per-position check)
  // LEAN Solve (KS_TPL_MEMO): what the last NewNodeClaim from a template without a NodePool limit derived, keyed by
  // (template, pod requests): options, thresholds, option count, max Allocatable (try_templates)
  enum : int { MM_T = 0, MM_CNT, MM_FOK, MM_POD = 4 };  // then [R] pod, [R] max (int64), [R] thr, [TW] options
  static constexpr bool TPL_MEMO = KS_TPL_MEMO && LEAN && !SIM;
  LU32 s_memo;          // [tpl_memo_words]
  int64_t memoHits = 0;
  // LEAN Solve (KS_TPL_MASKS, when the plan holds the table: pl.tmask): per template without a NodePool limit, what
  // filterInstanceTypesByRequirements' requirement and offering tests give for every position -- a function of the
  // template alone here (try_templates).  Row t: [TW] Intersects, [TW] hasOffering; s_tmv[t]: the row is filled.
  static constexpr bool TPL_MASKS = KS_TPL_MASKS && LEAN && !SIM;
  LU32 s_tmask;         // [NTPL][2 * TW]
  LU32 s_tmv;           // [NTPL]
  int64_t maskFills = 0, maskHits = 0;
  // LEAN Solve (KS_TPL_TABLE, when the handle holds the table: ks_problem.h): a NewNodeClaim that misses the memo under
  // the memo's conditions copies k_fresh_claims' record of (the pod's request class, t) into s_memo and goes on as a hit
  static constexpr bool TPL_TABLE = KS_TPL_TABLE && !KS_TPL_MASKS && TPL_MEMO;
  static constexpr bool TPL_TABLE_CHECK = KS_TPL_TABLE_CHECK && TPL_TABLE;
  // (its counter is a member of the LEAN Solve alone: the other instantiations' Solver keeps its layout)
  struct TableHits { int64_t n = 0; };
  struct NoTableHits {};
  [[no_unique_address]] std::conditional_t<TPL_TABLE, TableHits, NoTableHits> tableHits;
  // LEAN Solve (KS_RUN_FRONT): the templates' Pareto fronts (KsDev::tpl_front), and per LDS-resident claim whether
  // its options held every front member that fitted its first requests (try_templates): bit TPL_FOK of lc.tpl
  static constexpr bool RUN_FRONT = KS_RUN_FRONT && KS_CLAIM_RUNS && LEAN && !SIM;
  enum : int { TPL_FOK = 1 << 30 };
  static __device__ __forceinline__ int tplv(int x) { return RUN_FRONT ? x & ~(int)TPL_FOK : x; }
  LI32 s_fbeg;          // [NTPL+1]
  LI32 s_front;         // [frontTotal] template positions
  mutable int64_t capFront = 0, capFull = 0;  // claim_run_cap calls by path
  // LEAN Solve (KS_CAP_BOUND): commit_claim notes whether the pod exceeds the headroom it stores in some resource;
  // the run that would follow then has capacity 0 and claim_run_cap is not called (capBoundSkips)
  static constexpr bool CAP_BOUND = KS_CAP_BOUND && KS_CLAIM_RUNS && LEAN && !SIM;
  // LEAN Solve (KS_RUN_CHAIN): a pod identical to the one a NodeClaim just took skips the node phase (ks_solve_body.inc)
  static constexpr bool RUN_CHAIN = KS_RUN_CHAIN && KS_CLAIM_RUNS && LEAN && !SIM;
  bool capOver = false;
  int64_t capBoundSkips = 0;
  // LEAN Solve (KS_THR_BATCH): claim_full calls whose threshold advance took the batched first chunk, and those of
  // them in which one resource dropped more than 64 options (the per-resource loop went on)
  static constexpr bool THR_BATCH = KS_THR_BATCH && LEAN && !SIM;
  int64_t thrBatchCalls = 0, thrMultiChunk = 0;
  LU32 s_rmv;           // SIM: [ceil(N/32)] nodes removed by the simulation (the candidates)
  LU32 s_tch;           // SIM: [ceil(N/32)] nodes whose requests live in a W.n_req slot
  LU32 s_tchr;          // SIM: [ceil(N/32)] nodes whose requirements live in a W.n_rs slot; Solve (d.fnOn): nodes
                        // whose requirements a commit narrowed (k_feasibility_nodes's bits no longer apply)
  LU32 s_tvol;          // SIM: [ceil(N/32)] nodes whose volume counts live in a W.n_vc slot (W.n_vslot)
  LI32 s_tgm;           // [G][TGM_WORDS] topology group metadata
  LI32 s_tmin;          // [G] domainMinCount of the popped pod, per spread group
  LU32 s_trs0;          // [RSW] AddRequirements' nodeRequirements snapshot
  LU32 s_trs1;          // [RSW] one group's domains as a single-key record
  LI32 s_tdom;          // [pl.tdl] the node domain table (a Solve whose table fits)
  LI32 s_tdw;           // SIM + TOPO: the register window's node domains, [key slot < kTdwKeys][kTdw]
  LI32 s_live;          // [pl.livl] a Solve's live node list (ks_solve_body.inc)
  LI32 s_tcs;           // [pl.tcl] the count table's LDS-resident prefix: the small-key groups (a Solve: the
                        // whole table when it fits, make_plan)
  LU32 s_tcd;           // SIM: dirty bits over count words [tgSmall, tgCntWords): set once W.tg_cnt holds the word
  // Topology-group sets are GMW-word bitsets (ks_problem.h).  Word 0 lives in a register (it is the whole set
  // whenever a problem has <= 64 groups); words 1.. live in LDS, s_gw[set * GMW + w] (sets GS_*).
  LU64 s_gw;            // [GS_N][GMW] when GMW > 1
  uint64_t t_mask = 0;  // groups matching the popped pod (owned in its state | inverse groups selecting it), word 0
  uint64_t t_sel = 0;   // groups whose selector selects the popped pod, word 0
  uint64_t t_inv = 0;   // inverse groups the popped pod owns, word 0
  bool t_any = false;   // t_mask is not empty (any word)
  bool t_rec = false;   // t_sel | t_inv is not empty (any word): Topology.Record has groups to visit
  int t_s = 0;          // the popped pod's relaxation state
  uint64_t t_rss = 0;   // keys the state's strict pod requirements name (rs_present of its st_rss row)
  const uint32_t KS_G* fnp = nullptr;  // k_feasibility_nodes's row of the popped pod's state (null: none)
  bool t_nonode = false;  // some matching group admits no domain at all: no existing node can pass
  uint64_t t_active = ~0ull;  // groups in t.topologies so far (late groups join at their relaxation), word 0
  int64_t algbytes = 0;
  bool rem_same = false;  // the last claim_full left the claim's options unchanged (commit skips the copy back)
  uint64_t cur_hpc = 0, cur_hpu = 0;  // the popped pod's host-port conflict / reservation masks
  uint64_t cur_hpo = 0;               // its own initial entries on existing nodes (HostPortUsage.Add replaces them)
  // the popped pod's volumes (volA), in LDS (SGPRs are the scarce resource of the non-LEAN loop): driver
  // entries [VO_DB, VO_DE) of D.pod_vd, NewScheduler-time mounts of its PVCs [VO_SB, VO_SE) of D.pod_vs, this
  // Solve's earlier mounts of them [0, VO_NSP) of W.vspec (PF_VSHARED pods: its PVCs [VO_UB, VO_UE) of
  // D.pod_vu); VO_NLOG entries in W.vlog; SIM: VO_NSLOT W.n_vc slots in use
  enum : int { VO_DB = 0, VO_DE, VO_SB, VO_SE, VO_NSP, VO_UB, VO_UE, VO_NLOG, VO_NSLOT, VO_WORDS };
  LI32 s_vol;
#ifdef KS_PHASE_STATS
  mutable uint64_t scyc[4] = {0, 0, 0, 0};  // claim_full sub-phases: requirements, thresholds, masks, apply
  mutable uint64_t xcyc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // the step's sub-phases (StepSub)
  uint64_t ecyc[3] = {0, 0, 0};  // the exact re-sorts' cycles by size (CT_CYC_EXACT_BY_N)
  mutable uint64_t ycyc[6] = {0, 0, 0, 0, 0, 0};  // SS_TPL_DERIVE and SS_LOG split (SplitSub)
  mutable uint64_t kcyc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // the steps by kind, threshold moves, empty runs (KindSub)
  mutable uint64_t zcyc[3] = {0, 0, 0};  // inside cycSort and cycCross: pivot samples, regather, quick re-tests (ResortSub)
#endif

  __device__ Solver(const KsDev& D_, const KsWork KS_C& W_, const Plan& p_) : D(D_), d(D_.d), W(W_), pl(p_) {}
  __device__ __forceinline__ int R() const { return RT > 0 ? RT : d.R; }

  template <bool INL>
  __device__ __forceinline__ const ClaimView<INL>& cv() const {
    if constexpr (INL) return lc;
    else return gc;
  }

  template <class P>
  __device__ __forceinline__ bool fits(const int64_t* req, P alloc) const {  // resources.go:162-175
    bool ok = true;
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      const int64_t a = alloc[r];
      ok &= (a >= 0) & (req[r] <= a);
    }
    return ok;
  }
  __device__ __forceinline__ bool fits_pos(const int64_t* req, int gpos) const {
    if constexpr (TL) return fits(req, s_talloc + (int64_t)gpos * R());
    else return fits(req, D.it_alloc + (int64_t)D.tpl_its[gpos] * R());
  }
  __device__ __forceinline__ int64_t alloc_pos(int gpos, int r) const {
    if constexpr (TL) return s_talloc[(int64_t)gpos * R() + r];
    else return D.it_alloc[(int64_t)D.tpl_its[gpos] * R() + r];
  }
  __device__ __forceinline__ int64_t tsort_a(int64_t i) const {
    if constexpr (TL) return s_tsa[i];
    else return D.tsort_alloc[i];
  }
  __device__ __forceinline__ int tsort_p(int64_t i) const {
    if constexpr (TL) return s_tsp[i];
    else return D.tsort_pos[i];
  }

  // Commit log (scheduler.go:253/274 placements in order): lane (i & 63) holds entry i until 64 are
  // buffered, then one coalesced store.  Per-pod global stores would make the next global load wait
  // for their write acknowledgements (vmcnt counts stores on gfx9).
  int lg_p = 0, lg_t = 0;
  // LEAN Solve (KS_LOG_RUNS): entries of run records belong to k_log_expand.  lg_lo: the buffered block's lanes
  // before it were stored already (flushed ahead of a record) or are a record's; every block store is masked to
  // the lanes from it on, so this kernel and k_log_expand write disjoint entries.
  static constexpr bool LOG_RUNS = KS_LOG_RUNS && KS_CLAIM_RUNS && LEAN && !SIM;
  int lg_lo = 0;
  int runRecs = 0;
  // (A pass's simulations only count their placements: the host reads their records.  SLOG: the re-run of one
  // simulation whose placements the host renders stores them as a Solve does, ks_simlog.hip.)
  __device__ __forceinline__ void log_commit(int p, int tgt, int& nlog) {
    if constexpr (SIM && !SLOG) {
      nlog++;
      return;
    }
    if (lane() == (nlog & (kWave - 1))) {
      lg_p = p;
      lg_t = tgt;
    }
    nlog++;
    if ((nlog & (kWave - 1)) == 0) {
      if (!LOG_RUNS || lane() >= lg_lo) {
        W.log_pod[nlog - kWave + lane()] = lg_p;
        W.log_tgt[nlog - kWave + lane()] = lg_t;
      }
      if constexpr (LOG_RUNS) lg_lo = 0;
    }
  }
  // Commit-log entries for `n` (<= 64) placements at once: lane t holds entry nlog + t (pod, target).
  // Its callers are the NodeClaim runs, which are a Solve's alone (LEAN && !SIM): no SLOG instantiation reaches it
  // (a logged simulation's pods all go through log_commit), so the gate below only keeps the three functions alike.
  __device__ __forceinline__ void log_batch(int n, int pod_t, int tgt_t, int& nlog) {
    if constexpr (SIM && !SLOG) {
      nlog += n;
      return;
    }
    const int b0 = nlog & (kWave - 1);
    const int src = (lane() - b0) & (kWave - 1);  // the entry this lane buffers: nlog + src
    const int pv = __shfl(pod_t, src), tv = __shfl(tgt_t, src);
    const bool mine = src < n;
    if (mine && lane() >= b0) {
      lg_p = pv;
      lg_t = tv;
    }
    if (b0 + n >= kWave) {  // the buffered block is complete: store it, then buffer the wrapped entries
      if (!LOG_RUNS || lane() >= lg_lo) {
        W.log_pod[nlog - b0 + lane()] = lg_p;
        W.log_tgt[nlog - b0 + lane()] = lg_t;
      }
      if constexpr (LOG_RUNS) lg_lo = 0;
      if (mine && lane() < b0) {
        lg_p = pv;
        lg_t = tv;
      }
    }
    nlog += n;
  }
  __device__ __forceinline__ void log_flush(int nlog) {
    if constexpr (SIM && !SLOG) return;
    const int k = nlog & (kWave - 1);
    if (lane() < k && (!LOG_RUNS || lane() >= lg_lo)) {
      W.log_pod[nlog - k + lane()] = lg_p;
      W.log_tgt[nlog - k + lane()] = lg_t;
    }
  }
  // A run of k pods from queue position qhead on claim c, the queue being NewQueue's order: one record.  The
  // buffered entries before it are stored first, so that everything from nlog to nlog + k is k_log_expand's.
  __device__ __forceinline__ void log_run_record(int k, int qhead, int c, int& nlog) {
    log_flush(nlog);
    if (lane() < 4)
      W.run_log[4 * runRecs + lane()] = lane() == 0 ? nlog : lane() == 1 ? qhead : lane() == 2 ? k : c;
    runRecs++;
    nlog += k;
    lg_lo = nlog & (kWave - 1);
  }
  template <class PR>
  __device__ __forceinline__ bool has_offering(int it, PR rs) const {  // nodeclaim.go:270-278
    const int b = D.it_off_beg[it], e = D.it_off_beg[it + 1];
    for (int o = b; o < e; o++)
      if (rs_member(L, rs, d.zoneKey, D.off_zone[o]) && rs_member(L, rs, d.ctKey, D.off_ct[o])) return true;
    return false;
  }
  // filterInstanceTypesByRequirements' requirement and offering tests (nodeclaim.go:225-278) for every
  // position of template t at once, from the host's per-(key, value) position bitsets (ks_host.cpp
  // "feasibility tables"): for each key of X that instance types constrain, Requirements.Intersects
  // passes on the positions whose IT lacks the key (only shared keys are checked), on those holding a
  // value X admits, and -- when X's operator is NotIn / DoesNotExist -- on those whose IT says
  // DoesNotExist (both negative, requirements.go:248-252); the keys intersect.  hasOffering is the union
  // over the (zone, capacity-type) pairs X admits (a missing key admits all).  Lane w owns word w:
  // s_fic, s_fof; s_firr marks positions whose IT holds a complement requirement (checked exactly).
  // fmrow: k_feasibility's row for (the popped pod's state, t) -- the keys no instance type constrains
  // with more than one value, already intersected for the template and the state -- when X is the
  // template's or a claim's requirements plus that state's (Compatible with it) and nothing else: per
  // such key the test factorises for the value positions (an IT's single value is admitted by X = A + B
  // iff by A and by B), and the claim's options already satisfy A's part.  An IT's DoesNotExist does not
  // factorise (Exists + NotIn is NotIn, which it intersects, requirements.go:248-252): the row passes
  // those positions and they are tested here against X's operator.  Only the multi-valued keys are
  // evaluated in full then.
  __device__ __forceinline__ void feas_masks(LU32 X, int t, const uint32_t KS_G* fmrow = nullptr) {
    const uint32_t KS_G* F = D.fk_words;
    const int TW = d.TW;
    const int ball = D.fk_tpl[3 * t], birr = D.fk_tpl[3 * t + 1], boff = D.fk_tpl[3 * t + 2];
    const uint64_t keysX = rs_present(X) & d.itKeys & (fmrow ? d.fkMulti : ~0ull);
    uint64_t keysDne = 0;  // fmrow: X's single-valued IT keys whose operator is In / Exists
    if (fmrow)
      for (uint64_t m = rs_present(X) & d.itKeys & ~d.fkMulti; m; m &= m - 1) {
        const int op = rs_op(L, X, ctz64(m));
        if (op != OP_NOTIN && op != OP_DNE) keysDne |= m & (~m + 1);
      }
    const int nz = L.keys[d.zoneKey].nv, nc = L.keys[d.ctKey].nv;
    for (int w0 = 0; w0 < TW; w0 += kWave) {
      const int w = w0 + lane();
      const int wc = w < TW ? w : TW - 1;
      uint32_t ic = F[ball + wc] & fk_intersects_word(D, L, X, t, wc, keysX);
      if (fmrow) {
        ic &= fmrow[wc];
        // the row passes DoesNotExist positions; they intersect X iff X's operator is negative there
        for (uint64_t m = keysDne; m; m &= m - 1) ic &= ~F[D.fk_key_off[t * d.NK + ctz64(m)] + TW + wc];
      }
      uint32_t of = 0;
      for (int c0 = 0; c0 < nc; c0 += kWave) {
        const uint64_t cm0 = wballot(c0 + lane() < nc && rs_member(L, X, d.ctKey, c0 + lane()));
        if (!cm0) continue;
        for (int z0 = 0; z0 < nz; z0 += kWave) {
          for (uint64_t zm = wballot(z0 + lane() < nz && rs_member(L, X, d.zoneKey, z0 + lane())); zm; zm &= zm - 1) {
            const int z = z0 + ctz64(zm);
            for (uint64_t cm = cm0; cm; cm &= cm - 1) of |= F[boff + (z * nc + c0 + ctz64(cm)) * TW + wc];
          }
        }
      }
      const uint32_t irr = F[birr + wc];
      if (w < TW) {
        s_fic[w] = ic;
        s_fof[w] = of;
        s_firr[w] = irr;
      }
    }
    wsync();
  }
  // k_feasibility's row for (state s, template t), or null where it does not apply: not computed, or
  // topology requirements were added to the record (they are not part of the row).
  __device__ __forceinline__ const uint32_t KS_G* fm_row(int s, int t) const {
    if (KS_FM_OFF || !d.fmOn || (TOPO && t_any)) return nullptr;
    return D.st_fm + ((int64_t)s * d.NTPL + t) * d.TW;
  }
  __device__ __forceinline__ bool fbit(LU32 m, int pos) const { return (m[pos >> 5] >> (pos & 31)) & 1u; }

  template <class PD, class PS>
  __device__ __forceinline__ void copy_words(PD dst, PS src, int n) const {
    for (int i = lane(); i < n; i += kWave) dst[i] = src[i];
  }
  __device__ __forceinline__ void store_bits(LU32 dst, int base, uint64_t m) const {
    if (lane() == 0) {
      dst[base >> 5] = (uint32_t)m;
      if ((base >> 5) + 1 < d.TW) dst[(base >> 5) + 1] = (uint32_t)(m >> 32);
    }
  }
  __device__ __forceinline__ int popc_words(LU32 w, int n) const {
    int c = 0;
    for (int i = lane(); i < n; i += kWave) c += __popc(w[i]);
    return wred_add(c);
  }


  // --- existing nodes (ExistingNode.Add, existingnode.go:64-124) -------------------------------
  // Volumes (VolumeUsage, volumeusage.go:183-227; KsDev in ks_problem.h).  vol_pop loads the popped pod's
  // entries (wave-uniform); for a pod sharing a PVC with other pods being scheduled it also collects the
  // earlier placements' log entries of its PVCs (W.vlog -> W.vspec; every store here is a wave-wide store of
  // a uniform value, so each lane later reads what it wrote itself).
  __device__ __forceinline__ int vo(int f) const { return uni(s_vol[f]); }
  __device__ __forceinline__ void vo_set(int f, int v) const { s_vol[f] = v; }  // wave-wide store of a uniform value
  __device__ __forceinline__ void vol_pop(int g, int pf) {
    vo_set(VO_DB, D.pod_vdbeg[g]);
    vo_set(VO_DE, D.pod_vdbeg[g + 1]);
    vo_set(VO_SB, D.pod_vsbeg[g]);
    vo_set(VO_SE, D.pod_vsbeg[g + 1]);
    int ub = 0, ue = 0, nsp = 0;
    if (pf & PF_VSHARED) {
      ub = uni(D.pod_vubeg[g]);
      ue = uni(D.pod_vubeg[g + 1]);
      const int nlog = vo(VO_NLOG);
      for (int i0 = 0; i0 < nlog; i0 += kWave) {
        const int i = i0 + lane();
        const int ic = i < nlog ? i : i0;
        const int lu = W.vlog[2 * ic], ln = W.vlog[2 * ic + 1];
        bool hit = false;
        for (int k = ub; k < ue; k++) hit |= D.pod_vu[k] == lu;
        for (uint64_t m = wballot(hit && i < nlog); m; m &= m - 1) {
          const int l = ctz64(m);
          W.vspec[2 * nsp] = rdl(lu, l);  // wave-wide stores of uniform values
          W.vspec[2 * nsp + 1] = rdl(ln, l);
          nsp++;
        }
      }
    }
    vo_set(VO_UB, ub);
    vo_set(VO_UE, ue);
    vo_set(VO_NSP, nsp);
    wsync();
  }
  __device__ __forceinline__ bool vol_any() const { return vo(VO_DE) > vo(VO_DB); }
  // The pod's PVCs of driver v that node n mounts already (at NewScheduler time, or by an earlier placement).
  __device__ __forceinline__ int vol_mounted(int n, int v) const {
    int c = 0;
    for (int k = vo(VO_SB), e = vo(VO_SE); k < e; k++) c += (D.pod_vs[2 * k] == n && D.vol_udrv[D.pod_vs[2 * k + 1]] == v) ? 1 : 0;
    for (int k = 0, e = vo(VO_NSP); k < e; k++) c += (W.vspec[2 * k + 1] == n && D.vol_udrv[W.vspec[2 * k]] == v) ? 1 : 0;
    return c;
  }
  __device__ __forceinline__ const int32_t KS_G* vol_row(int n) const {
    if (!SIM) return W.n_vc + (int64_t)n * d.VD;
    return tbit(s_tvol, n) ? W.n_vc + (int64_t)W.n_vslot[n] * d.VD : D.n_vc0 + (int64_t)n * d.VD;
  }
  // VolumeUsage.ExceedsLimits (volumeusage.go:202-209) of the popped pod on node n (per lane): per limited
  // driver it mounts, the node's count plus its PVCs the node does not mount yet.
  __device__ __forceinline__ bool vol_ok(int n) const {
    const int32_t KS_G* vc = vol_row(n);
    bool ok = true;
    for (int j = vo(VO_DB), e = vo(VO_DE); j < e; j++) {
      const int v = D.pod_vd[2 * j], c = D.pod_vd[2 * j + 1];
      ok &= vc[v] + c - vol_mounted(n, v) <= D.n_vlim[(int64_t)n * d.VD + v];
    }
    return ok;
  }
  // VolumeUsage.Add (existingnode.go:122) of the popped pod on node n (wave-uniform n; wave-wide stores of
  // uniform values).  SIM: the node's counts move to a W.n_vc slot at its first such placement.
  __device__ __forceinline__ void vol_commit(int n) {
    int32_t KS_G* vc;
    if (SIM) {
      if (!tbit(s_tvol, n)) {
        const int slot = vo(VO_NSLOT);
        for (int v = 0; v < d.VD; v++) W.n_vc[(int64_t)slot * d.VD + v] = D.n_vc0[(int64_t)n * d.VD + v];
        W.n_vslot[n] = slot;
        vo_set(VO_NSLOT, slot + 1);
        __hip_atomic_fetch_or(s_tvol + (n >> 5), 1u << (n & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        wsync();
        vc = W.n_vc + (int64_t)slot * d.VD;
      } else {
        vc = W.n_vc + (int64_t)uni(W.n_vslot[n]) * d.VD;
      }
    } else {
      vc = W.n_vc + (int64_t)n * d.VD;
    }
    for (int j = vo(VO_DB), e = vo(VO_DE); j < e; j++) {
      const int v = D.pod_vd[2 * j], c = D.pod_vd[2 * j + 1];
      const int add = uni(c - vol_mounted(n, v));
      if (add) vc[v] = uni(vc[v]) + add;
    }
    // the shared pod's PVCs not yet on n join the log (each (PVC, node) pair once)
    int nlog = vo(VO_NLOG);
    for (int k = vo(VO_UB), e = vo(VO_UE); k < e; k++) {
      const int u = D.pod_vu[k];
      bool on = false;
      for (int q = vo(VO_SB), qe = vo(VO_SE); q < qe; q++) on |= D.pod_vs[2 * q] == n && D.pod_vs[2 * q + 1] == u;
      for (int q = 0, qe = vo(VO_NSP); q < qe; q++) on |= W.vspec[2 * q + 1] == n && W.vspec[2 * q] == u;
      if (!ub(on)) {
        W.vlog[2 * nlog] = u;
        W.vlog[2 * nlog + 1] = n;
        nlog++;
      }
    }
    vo_set(VO_NLOG, nlog);
    hbm_release();
    wsync();
  }
  // Lane (n & 63) is the only lane that ever reads or writes node n's mutable state.
  __device__ __forceinline__ bool tbit(LU32 m, int n) const { return (m[n >> 5] >> (n & 31)) & 1u; }
  // Existing-node check for KN nodes per lane (positions n, n + 64, ... of the first-fit order): every
  // load of all of them is issued before any test, so a (KN * 64)-node step of the scan costs one memory
  // round trip (two with topology: the nodes' domains, then their counts).  Out-of-range positions are
  // clamped for the loads and masked.  nf: NodeFlag bits.  sl[i]: the node passed every check but lacks
  // the label of a matching group's key, so only the wave-cooperative node_slow can decide it (ok is
  // false then).
  // LIST: lane l of block i tests node nl[i] (the Solve's live list; -1: none) instead of n0 + 64 i + l; stay[i]:
  // the node still passes Fits for these requests once the pod is committed to it (the list keeps it).
  template <int KN, bool LIST = false>
  __device__ __forceinline__ void node_okK(int n0, int sflags, const int64_t* pod, uint64_t tol0, uint64_t tol1,
                                           bool* ok, int* nf, int64_t (*q)[RM], bool* sl, bool* rk,
                                           const int* nl = nullptr, bool* stay = nullptr) const {
    int c[KN];
    uint64_t tx[KN], ty[KN], h[KN];
    int64_t a[KN][RM];
    PH_BEGIN(tok);
#pragma unroll
    for (int i = 0; i < KN; i++) {
      const int n = LIST ? nl[i] : n0 + i * kWave;
      c[i] = LIST ? (n >= 0 ? n : 0) : n < d.N ? n : d.N - 1;
      const bool own = !SIM || tbit(s_tch, c[i]);
      const uint64_t KS_G* tp = D.n_taint + 2 * c[i];
      const int64_t KS_G* ap = D.n_avail + (int64_t)c[i] * R();
      const int64_t KS_G* qp = (own ? W.n_req : D.n_req0) + (int64_t)c[i] * R();
      tx[i] = tp[0];
      ty[i] = tp[1];
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= d.R) break;
        a[i][r] = ap[r];
        q[i][r] = qp[r];
      }
      nf[i] = SIM ? D.n_flags[c[i]] : 0;
      h[i] = 0;
      if (hpA()) h[i] = own ? W.n_hp[c[i]] : D.n_hp0[c[i]];  // HostPortUsage.Conflicts (hostportusage.go:74-85)
    }
#pragma unroll
    for (int i = 0; i < KN; i++) {
      bool rr = LIST ? nl[i] >= 0 : n0 + i * kWave < d.N;
      if (SIM) rr &= !tbit(s_rmv, c[i]);  // the simulation removed these candidates
      bool st = true;
#pragma unroll
      for (int r = 0; r < RM; r++) {  // Fits(requests + pod, Available())
        if (RT == 0 && r >= d.R) break;
        rr &= (a[i][r] >= 0) & (q[i][r] + pod[r] <= a[i][r]);
        if (LIST) st &= q[i][r] + 2 * pod[r] <= a[i][r];
      }
      if (LIST) stay[i] = st;
      rk[i] = rr;  // (permanent for these requests: the caller's resource-failing prefix)
      ok[i] = rr & (((tx[i] & ~tol0) | (ty[i] & ~tol1)) == 0) & ((h[i] & cur_hpc) == 0);  // Taints.Tolerates
      if (volA() && vol_any() && ok[i]) ok[i] = vol_ok(c[i]);
      if (keys(sflags) && ok[i]) ok[i] = node_compat(c[i]);  // strict Compatible
      sl[i] = false;
    }
    PH_BEGIN(ttp);
    if (TOPO && t_any) topo_node_stateK<KN>(c, ok, sl);  // topology (existingnode.go:106-114)
    if (LIST) PHS_END(ttp, 1);  // stats build: its topology tests
  }
  __device__ __forceinline__ const uint32_t KS_G* node_rs(int n) const {
    if (!SIM) return W.n_rs + (int64_t)n * d.RSW;
    return tbit(s_tchr, n) ? W.n_rs + (int64_t)W.n_slot[n] * d.RSW : D.n_rs0 + (int64_t)n * d.RSW;
  }
  // ExistingNode.Add's strict Compatible(node requirements, pod requirements) (existingnode.go:97-104) for
  // node n: k_feasibility_nodes's bit while the node keeps its initial record (that bit also ANDs the
  // taint test the caller already applied), else the exact test on the node's current record.
  __device__ __forceinline__ bool node_compat(int n) const {
    if (fnp && !tbit(s_tchr, n)) return (fnp[n >> 5] >> (n & 31)) & 1u;
    return rs_compatible(L, node_rs(n), s_pin, 0);
  }
  // Solve (d.fnOn): node j's requirements were narrowed by a commit; its row bit no longer applies.
  __device__ __forceinline__ void node_rs_changed(int j) const {
    if (!SIM && d.fnOn)
      __hip_atomic_fetch_or(s_tchr + (j >> 5), 1u << (j & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
  }
  // Solve: commit of a pod to node j by its owner lane.
  __device__ __forceinline__ void node_commit(int j, int s, int sflags, const int64_t* pod) {
    for (int r = 0; r < R(); r++) W.n_req[(int64_t)j * R() + r] += pod[r];
    if (hpA()) W.n_hp[j] = (W.n_hp[j] & ~cur_hpo) | cur_hpu;  // HostPortUsage.Add (hostportusage.go:70-72)
    if (keys(sflags)) {
      rs_add(L, W.n_rs + (int64_t)j * d.RSW, s_pin);
      node_rs_changed(j);
    }
  }
  // SIM: copy-on-write commit (wave-uniform).  W.n_req is indexed by node but only the nodes a pod
  // landed on are ever written (s_tch marks them), so a fresh simulation needs no initialisation.
  // Requirements are copied only when a pod with label requirements lands, into the next compact
  // slot of W.n_rs (wave-cooperatively, through LDS).
  // `q`: the owner lane's requests of node j as node_okK loaded them (no reload before the store).
  // regReq: node j sits in the register window (its requests are updated there, not in HBM).
  __device__ __forceinline__ void sim_node_commit(int j, int s, int sflags, const int64_t* pod, const int64_t* q,
                                                  int& nrs, bool regReq) {
    const int owner = j & (kWave - 1);
    const bool fresh = !tbit(s_tch, j);
    wsync();
    if (!regReq && lane() == owner) {
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= d.R) break;
        W.n_req[(int64_t)j * R() + r] = q[r] + pod[r];
      }
      if (hpA()) W.n_hp[j] = ((fresh ? D.n_hp0[j] : W.n_hp[j]) & ~cur_hpo) | cur_hpu;
      if (fresh) s_tch[j >> 5] |= 1u << (j & 31);
    }
    if (keys(sflags)) {
      const bool rsfresh = !tbit(s_tchr, j);
      int slot;
      if (rsfresh) {
        slot = nrs++;
        copy_words(s_rs, D.n_rs0 + (int64_t)j * d.RSW, d.RSW);
      } else {
        int v = 0;
        if (lane() == owner) v = W.n_slot[j];
        slot = rdl(v, owner);
        copy_words(s_rs, W.n_rs + (int64_t)slot * d.RSW, d.RSW);
      }
      wsync();
      rs_add_wave(L, s_rs, s_pin, 0);
      copy_words(W.n_rs + (int64_t)slot * d.RSW, s_rs, d.RSW);
      if (lane() == owner && rsfresh) W.n_slot[j] = slot;
      if (lane() == 0) s_tchr[j >> 5] |= 1u << (j & 31);
      hbm_release();
    }
    wsync();
  }

  // --- Topology (topology.go, topologygroup.go) ------------------------------------------------
  // Counts and registered bits are written by one lane and read by others: loads bypass the L1.
  __device__ __forceinline__ int tg(int g, int f) const { return s_tgm[g * TGM_WORDS + f]; }
  // count of domain v, -1 while the domain is not registered (absent from TopologyGroup.domains)
  // Small-key groups read LDS.  The hostname groups (one word per node) live in HBM: a Solve's workspace
  // holds a full copy (k_init); a simulation reads the shared NewTopology counts until it first writes a
  // word (copy-on-write, s_tcd), so no simulation copies the table.
  __device__ __forceinline__ int tcnt_at(int off) const {
    if (off < pl.tcl) return s_tcs[off];
    if constexpr (SIM) {
      const int b = off - d.tgSmall;
      const int own = ld_sc1(W.tg_cnt + off), shared = D.tg_cnt0[off];
      return ((s_tcd[b >> 5] >> (b & 31)) & 1u) ? own : shared;
    }
    return ld_sc1(W.tg_cnt + off);
  }
  __device__ __forceinline__ int tcnt(int g, int v) const { return tcnt_at(tg(g, TGM_CNT) + v); }
  // node n's domain of group g's key (-1: the node lacks the label): LDS in a Solve whose table fits, and for
  // a topology simulation's register-window nodes (the first kTdw nodes: every scan starts there)
  __device__ __forceinline__ int tdom(int g, int n) const {
    if constexpr (SIM && TOPO)
      if (n < kTdw && tg(g, TGM_KSLOT) < kTdwKeys) return s_tdw[tg(g, TGM_KSLOT) * kTdw + n];
    const int off = tg(g, TGM_KSLOT) * d.N + n;
    return off < pl.tdl ? s_tdom[off] : D.n_tdom[off];
  }
  // Topology.Record's count increment of word `off` (recording registers the domain), by one lane;
  // concurrent callers touch distinct words.
  __device__ __forceinline__ void tcnt_inc(int off) const {
    const int c = tcnt_at(off);
    const int n = c < 0 ? 1 : c + 1;
    if (off < pl.tcl) {
      s_tcs[off] = n;
      return;
    }
    W.tg_cnt[off] = n;
    if constexpr (SIM) {
      const int b = off - d.tgSmall;
      __hip_atomic_fetch_or(s_tcd + (b >> 5), 1u << (b & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
  }
  __device__ __forceinline__ int tccnt(int g, int claim) const { return ld_sc1(W.tg_ccnt + (int64_t)g * W.ccs + claim); }  // claim <= Kcap (a fresh claim at the cap)
  // podDomains.Has (strict pod requirements).  A key the pod's strict requirements do not name admits every value
  // (Get() of a missing key is Exists), which is the common case: the row's presence mask (t_rss, read with the
  // pop's other group words) answers it without a load.
  __device__ __forceinline__ bool tpod_has(int g, int v) const {
    const int k = tg(g, TGM_KEY);
    if (!((t_rss >> k) & 1ull)) return true;
    return rs_member(L, D.st_rss + (int64_t)t_s * d.RSW, k, v);
  }
  // Per pop: the matching groups (getMatchingTopologies, topology.go:366-379: owned groups, then
  // inverse groups whose selector selects the pod), domainMinCount per spread group (:192-213) and,
  // per affinity group, whether some domain the pod allows already holds a selected pod (:215-221;
  // for hostname keys that includes NodeClaim placeholders, counted in tg_cpos).
  // Word w of the set {0, ..., n-1}.
  __device__ __forceinline__ static uint64_t bits_below(int n, int w) {
    const int k = n - 64 * w;
    return k >= 64 ? ~0ull : k <= 0 ? 0ull : ((1ull << k) - 1ull);
  }
  // Word w of group set `set` (GS_*); r0: the set's register word 0.
  __device__ __forceinline__ uint64_t gword(int set, int w, uint64_t r0) const {
    return w == 0 ? r0 : (uint64_t)uni64((int64_t)s_gw[set * d.GMW + w]);
  }
  __device__ __forceinline__ bool sel_has(int g) const {  // the popped pod is selected by group g
    return ((gword(GS_SEL, g >> 6, t_sel) >> (g & 63)) & 1ull) != 0;
  }
  // sel0 / inv0 / own0 / rss0: word 0 of the pod's group sets and its strict keys, gathered with the queue
  // window (refill), so a pop's group evaluation starts without a memory round trip
  __device__ __forceinline__ void topo_pop(int s, int gpod, uint64_t sel0, uint64_t inv0, uint64_t own0, uint64_t rss0) {
    t_s = s;
    const int GMW = d.GMW;
    const uint64_t KS_G* sel = D.pod_gsel + (int64_t)gpod * GMW;
    const uint64_t KS_G* inv = D.pod_ginv + (int64_t)gpod * GMW;
    const uint64_t KS_G* own = D.st_gown + (int64_t)s * GMW;
    t_sel = sel0;
    t_inv = inv0;
    t_rss = rss0;
    t_mask = own0 | (t_sel & bits_below(d.G, 0) & ~bits_below(d.G1, 0));
    if (SIM) t_mask &= ~W.tdead[0];
    bool anyM = t_mask != 0, anyR = (t_sel | t_inv) != 0;
    if (GMW > 1) {  // words 1.. (more than 64 groups), one lane each, into LDS
      bool m = false, r = false;
      for (int w = 1 + lane(); w < GMW; w += kWave) {
        const uint64_t sw = sel[w], iw = inv[w];
        uint64_t mw = own[w] | (sw & bits_below(d.G, w) & ~bits_below(d.G1, w));
        if (SIM) mw &= ~W.tdead[w];
        s_gw[GS_SEL * GMW + w] = sw;
        s_gw[GS_INV * GMW + w] = iw;
        s_gw[GS_MASK * GMW + w] = mw;
        m = m || mw != 0;
        r = r || (sw | iw) != 0;
      }
      anyM = anyM || wballot(m) != 0;
      anyR = anyR || wballot(r) != 0;
      wsync();
    }
    t_any = anyM;
    t_rec = anyR;
    t_nonode = false;
    for (int w = 0; w < GMW; w++)
      for (uint64_t m = gword(GS_MASK, w, t_mask); m; m &= m - 1) {
        const int g = 64 * w + ctz64(m);
        if (tg(g, TGM_TYPE) == TG_AFFINITY) {
          const int nv = tg(g, TGM_NV);
          bool pos = false, reg = false;
          for (int v = lane(); v < nv && !pos; v += kWave) {
            const int c = tcnt(g, v);
            const bool has = c >= 0 && tpod_has(g, v);
            pos = has && c > 0;
            reg = reg || has;
          }
          if (lane() == 0 && tg(g, TGM_HOST) && tpod_has(g, nv) && ld_sc1(W.tg_cpos + g) > 0) pos = true;
          const bool any = wballot(pos) != 0;
          s_tmin[g] = any ? 1 : 0;  // wave-wide store of a uniform value
          // topo_node_ok's test for this group over every domain: with a selected pod somewhere the
          // node's domain must hold one; otherwise only a self-selecting pod passes (a registered domain)
          if (!tg(g, TGM_HOST) && !any && !(sel_has(g) && wballot(reg))) t_nonode = true;
          continue;
        }
        if (tg(g, TGM_TYPE) == TG_ANTI) {  // topo_node_ok: the node's domain must hold no selected pod
          if (!tg(g, TGM_HOST)) {
            const int nv = tg(g, TGM_NV);
            bool ok = false;
            for (int v = lane(); v < nv && !ok; v += kWave) ok = tcnt(g, v) == 0 && tpod_has(g, v);
            if (!wballot(ok)) t_nonode = true;
          }
          continue;
        }
        if (tg(g, TGM_TYPE) != TG_SPREAD) continue;
        int mn = 0x7fffffff, num = 0;
        if (!tg(g, TGM_HOST)) {  // hostname groups always have a min of 0
          const int nv = tg(g, TGM_NV);
          int lo = 0x7fffffff;  // smallest registered count (any domain): topo_node_ok's best case
          for (int v = lane(); v < nv; v += kWave) {
            const int c = tcnt(g, v);
            if (c >= 0) lo = c < lo ? c : lo;
            if (c >= 0 && tpod_has(g, v)) {
              num++;
              mn = c < mn ? c : mn;
            }
          }
          mn = wred_min(mn, 0x7fffffff);
          lo = wred_min(lo, 0x7fffffff);
          num = wred_add(num);
          if (tg(g, TGM_MIND) >= 0 && num < tg(g, TGM_MIND)) mn = 0;
          const int self = sel_has(g) ? 1 : 0;
          if (lo == 0x7fffffff || (int64_t)lo + self - mn > tg(g, TGM_SKEW)) t_nonode = true;
        } else {
          mn = 0;
        }
        s_tmin[g] = mn;  // wave-wide store of a uniform value (mn is reduced over the wave)
      }
    wsync();
  }
  // ExistingNode.Add's topology step for node n (one lane each): a node's single domain of each matching group
  // must be the one TopologyGroup.Get returns (existingnode.go:106-114).  0 fails, 1 passes, 2: every labelled
  // group passes, but the node lacks the label of some group's key (its domain then comes from the
  // requirements it accumulated; node_slow decides).  The node scan's default, topo_node_stateK, applies these
  // tests group by group to a lane's KN nodes (their loads issued together); KS_TOPO_SEQ calls this per node.
  __device__ __forceinline__ int topo_node_state1(int n) const {
    int st = 1;
    for (int w = 0; w < d.GMW; w++)
      for (uint64_t m = gword(GS_MASK, w, t_mask); m; m &= m - 1) {
        const int g = 64 * w + ctz64(m);
        const int v = tdom(g, n);
        if (v < 0) {
          st = 2;
          continue;
        }
        const int c = tcnt(g, v);
        if (c < 0) return 0;  // unregistered: Get never returns it
        const int type = tg(g, TGM_TYPE);
        if (type == TG_SPREAD) {
          const int self = sel_has(g) ? 1 : 0;
          if ((int64_t)c + self - s_tmin[g] > tg(g, TGM_SKEW)) return 0;
        } else if (type == TG_AFFINITY) {  // a selected pod's domain, or the bootstrap for a self-selecting pod
          if (!tpod_has(g, v)) return 0;
          if (s_tmin[g] ? c == 0 : !sel_has(g)) return 0;
        } else if (c != 0 || !tpod_has(g, v)) {
          return 0;
        }
      }
    return st;
  }
  // KN nodes per lane, group by group: the KN domain and count loads of one group are issued together
  // (topo_node_state1's tests, state updated branch-free; KS_TOPO_SEQ: one node after the other).
  template <int KN>
  __device__ __forceinline__ void topo_node_stateK(const int* c, bool* ok, bool* sl) const {
#ifdef KS_TOPO_SEQ
#pragma unroll
    for (int i = 0; i < KN; i++) {
      const int st = ok[i] ? topo_node_state1(c[i]) : 0;
      ok[i] = st == 1;
      sl[i] = st == 2;
    }
#else
    int st[KN];
#pragma unroll
    for (int i = 0; i < KN; i++) st[i] = ok[i] ? 1 : 0;
    for (int w = 0; w < d.GMW; w++)
      for (uint64_t m = gword(GS_MASK, w, t_mask); m; m &= m - 1) {
        const int g = 64 * w + ctz64(m);
        int v[KN], cn[KN];
#pragma unroll
        for (int i = 0; i < KN; i++) v[i] = st[i] ? tdom(g, c[i]) : -1;
#pragma unroll
        for (int i = 0; i < KN; i++) cn[i] = v[i] >= 0 ? tcnt(g, v[i]) : 0;
        const int type = tg(g, TGM_TYPE), self = sel_has(g) ? 1 : 0, skew = tg(g, TGM_SKEW), mn = s_tmin[g];
#pragma unroll
        for (int i = 0; i < KN; i++) {
          const int vv = v[i] < 0 ? 0 : v[i];  // (v < 0 decides below; no out-of-range member test)
          bool pass;
          if (type == TG_SPREAD) pass = (int64_t)cn[i] + self - mn <= skew;
          else if (type == TG_AFFINITY) pass = tpod_has(g, vv) && (mn ? cn[i] != 0 : self != 0);
          else pass = cn[i] == 0 && tpod_has(g, vv);
          pass = pass && cn[i] >= 0;  // unregistered: Get never returns it
          const int nx = v[i] < 0 ? 2 : pass ? st[i] : 0;
          st[i] = st[i] == 0 ? 0 : nx;
        }
      }
#pragma unroll
    for (int i = 0; i < KN; i++) {
      ok[i] = st[i] == 1;
      sl[i] = st[i] == 2;
    }
#endif
  }
  // ExistingNode.Add's requirement and topology steps for node j, wave-wide, for a node lacking the
  // label of a matching group's key (existingnode.go:91-115): nodeRequirements = the node's requirements
  // + the pod's, then AddRequirements picks the domains over nodeRequirements.Get(key) exactly as for a
  // NodeClaim (a missing key reads as Exists, a pod's NotIn leaves the complement), and the strict
  // Compatible decides.  The other checks already passed.  On success s_rs holds the node's new
  // requirements (the pod's and the topology's added).
  __device__ __forceinline__ bool node_slow(int j, int s, int sflags) {
    wsync();
    copy_words(s_rs, node_rs(j), d.RSW);
    wsync();
    if (keys(sflags)) rs_add_wave(L, s_rs, s_pin, 0);
    return topo_apply(s_rs, -1, 0) == 0;
  }
  // The node's requirements after a node_slow commit (n.requirements = nodeRequirements): s_rs.
  // SIM: into the node's copy-on-write slot.
  __device__ __forceinline__ void node_store_rs(int j, int& nrs) {
    wsync();
    if (!SIM) {
      copy_words(W.n_rs + (int64_t)j * d.RSW, s_rs, d.RSW);
      if (lane() == 0) node_rs_changed(j);
    } else {
      const int owner = j & (kWave - 1);
      const bool rsfresh = !tbit(s_tchr, j);
      int slot;
      if (rsfresh) {
        slot = nrs++;
      } else {
        int v = 0;
        if (lane() == owner) v = W.n_slot[j];
        slot = rdl(v, owner);
      }
      copy_words(W.n_rs + (int64_t)slot * d.RSW, s_rs, d.RSW);
      if (lane() == owner && rsfresh) W.n_slot[j] = slot;
      if (lane() == 0) s_tchr[j >> 5] |= 1u << (j & 31);
    }
    hbm_release();
    wsync();
  }
  // Topology.AddRequirements + Compatible on a NodeClaim's candidate record `rs` (LDS), wave-wide.
  // Returns 0, FC_TOPO | group << 16, or FC_TOPO_COMPAT; on success rs holds the final requirements.
  // claim < 0: an existing node's record (node_slow; no hostname placeholder); allow: the final
  // Compatible's AllowUndefined keys (NodeClaim: well-known labels, nodeclaim.go:96; node: none).
  __device__ __forceinline__ uint32_t topo_apply(LU32 rs, int claim, uint64_t allow) {
    copy_words(s_trs0, rs, d.RSW);
    wsync();
    for (int w = 0; w < d.GMW; w++)
    for (uint64_t m = gword(GS_MASK, w, t_mask); m; m &= m - 1) {
      const int g = 64 * w + ctz64(m);
      const int k = tg(g, TGM_KEY), nv = tg(g, TGM_NV);
      const bool host = tg(g, TGM_HOST) != 0;
      const KeyMeta km = L.keys[k];
      const int nslot = nv + (host && claim >= 0 ? 1 : 0);  // + the claim's own hostname-placeholder (private bit)
      for (int i = lane(); i < d.RSW; i += kWave) s_trs1[i] = 0;
      wsync();
      // The values a domain scan visits.  When the record holds the key as an In set (a NodeClaim's
      // hostname: its own placeholder), Requirements.Add below keeps only values of that set (rs only
      // shrinks from the snapshot s_trs0), so the scan over the set's bits leaves rs exactly as the scan
      // over the whole universe would -- 5000 hostnames become one word per lane.
      const bool inSet = bit(rs_present(s_trs0), k) && !bit(rs_compl(s_trs0), k);
      auto scan = [&](bool restrict, auto&& body) {
        if (restrict && inSet) {
          for (int wd = lane(); wd < km.nw; wd += kWave)
            for (uint32_t x = s_trs0[L.HDR + km.off + wd]; x; x &= x - 1) {
              const int v = wd * 32 + __builtin_ctz(x);
              if (v < nslot) body(v);
            }
        } else {
          for (int v = lane(); v < nslot; v += kWave) body(v);
        }
      };
      if (tg(g, TGM_TYPE) == TG_SPREAD) {  // nextDomainTopologySpread: smallest count, then smallest name
        const int self = sel_has(g) ? 1 : 0, mn = s_tmin[g], skew = tg(g, TGM_SKEW);
        uint64_t best = ~0ull;
        scan(true, [&](int v) {
          const bool nodeHas = rs_member(L, s_trs0, k, v);
          int c = -1;
          if (nodeHas) c = v < nv ? tcnt(g, v) : tccnt(g, claim);  // placeholders are always registered
          const bool cand = c >= 0;
          c += self;
          if (cand && (int64_t)c - mn <= skew) {
            const uint64_t key = ((uint64_t)(uint32_t)c << 32) | (uint32_t)v;
            best = key < best ? key : best;
          }
        });
        best = wred_min(best, (uint64_t)~0ull);
        if (best == ~0ull) return FC_TOPO | ((uint32_t)g << 16);
        const int bv = (int)(uint32_t)best;
        if (lane() == 0) s_trs1[L.HDR + km.off + (bv >> 5)] = 1u << (bv & 31);
      } else if (tg(g, TGM_TYPE) == TG_AFFINITY) {  // nextDomainAffinity
        const bool self = sel_has(g);
        if (s_tmin[g]) {  // the domains already holding a selected pod (other placeholders drop out in Add)
          scan(true, [&](int v) {
            const int c = v < nv ? tcnt(g, v) : tccnt(g, claim);
            if (c > 0 && tpod_has(g, v))
              __hip_atomic_fetch_or(s_trs1 + L.HDR + km.off + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_WAVEFRONT);
          });
        } else if (self) {  // bootstrap: first registered pod∩node domain, then first registered pod domain
          // (canonical map order = sorted names = value order; for hostname keys the claim's own
          // placeholder is its only node domain, and any other insert drops out in Add)
          uint32_t z1 = ~0u, z2 = ~0u;
          for (int v = lane(); v < nslot; v += kWave) {
            const int c = v < nv ? tcnt(g, v) : tccnt(g, claim);  // a placeholder: -1 if not registered
            if (c < 0 || !tpod_has(g, v)) continue;
            if (v < nv) z2 = (uint32_t)v < z2 ? (uint32_t)v : z2;
            if (rs_member(L, s_trs0, k, v)) z1 = (uint32_t)v < z1 ? (uint32_t)v : z1;
            if (v >= nv) z2 = z2 == ~0u ? (uint32_t)v : z2;  // registered, so the options are not empty
          }
          z1 = wred_min(z1, ~0u);
          z2 = wred_min(z2, ~0u);
          if (z1 == ~0u && z2 == ~0u) return FC_TOPO | ((uint32_t)g << 16);
          if (lane() == 0) {
            if (z1 != ~0u) s_trs1[L.HDR + km.off + (z1 >> 5)] |= 1u << (z1 & 31);
            if (z2 != ~0u) s_trs1[L.HDR + km.off + (z2 >> 5)] |= 1u << (z2 & 31);
          }
        } else {
          return FC_TOPO | ((uint32_t)g << 16);
        }
      } else {  // nextDomainAntiAffinity: registered zero-count domains the pod's domains allow
        // (a Solve renders which check failed -- no zero-count domain at all vs none the record allows --
        // so only simulations, which report success alone, restrict this scan)
        bool any = false;
        scan(SIM, [&](int v) {
          bool in;
          if (v < nv) {
            in = tcnt(g, v) == 0 && tpod_has(g, v);
          } else {
            const bool has = tpod_has(g, v);
            any = any || has;  // some registered placeholder has a zero count (the fresh claim's, at least)
            in = has && tccnt(g, claim) == 0;
          }
          if (in) {
            __hip_atomic_fetch_or(s_trs1 + L.HDR + km.off + (v >> 5), 1u << (v & 31), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WAVEFRONT);
            any = true;
          }
        });
        if (wballot(any) == 0) return FC_TOPO | ((uint32_t)g << 16);
      }
      wsync();
      // requirements.Add(domains), run by every lane in lockstep on the same LDS words (wave-wide stores
      // of uniform values, see commit_claim)
      wr64(s_trs1, 0, 1ull << k);
      wsync();
      rs_add(L, rs, s_trs1);
      wsync();
    }
    // Compatible(nodeRequirements, topologyRequirements, AllowUndefinedWellKnownLabels)
    int ok = 1;
    if (lane() == 0) ok = rs_compatible(L, s_trs0, rs, allow) ? 1 : 0;
    ok = rdl(ok, 0);
    return ok ? 0u : (uint32_t)FC_TOPO_COMPAT;
  }
  // Topology.Record (topology.go:125-148) for the pod's final requirements F on NodeClaim `claim`,
  // or on existing node `node` (claim -1), wave-wide.  Only groups that count the pod are visited:
  // owned groups whose selector selects it, inverse groups it owns.  On an existing node F[key] is
  // the node's own label value (the strict Compatible admitted nothing else; ks_topo.cpp refuses
  // the one input where a pod's NotIn could stand in for a missing label), so the node's domain
  // table replaces the scan over F's value words.
  // Solve (not SIM): logAt >= 0 is the commit's log position; its log_hg entry gets the hostname groups Topology.Record
  // counted the pod in (the host replays them to print a hostname group's counts in an unsatisfiable-topology
  // message).
  template <class PR>
  __device__ __forceinline__ void topo_record(PR F, int claim, int node, uint64_t allow, int logAt) {
    hbm_release();
    const int GMW = d.GMW;
    if (node >= 0) {  // an existing node: one domain per group (its label); group 64 w + l in lane l
      for (int w = 0; w < GMW; w++) {
        const uint64_t sel = gword(GS_SEL, w, t_sel), inv = gword(GS_INV, w, t_inv), act = gword(GS_ACT, w, t_active);
        const uint64_t m = (sel & bits_below(d.G1, w) & act) | inv;
        if (!m) continue;
        bool mine = ((m >> lane()) & 1ull) != 0;
        const int g = mine ? 64 * w + lane() : 0;
        // a spread group over a filtered node set counts the pod only where the filter admits the node
        const bool filt = mine && g < d.G1 && tg(g, TGM_TYPE) == TG_SPREAD && tg(g, TGM_FEND) > tg(g, TGM_FBEG);
        for (uint64_t fm = wballot(filt); fm; fm &= fm - 1) {
          const int gf = 64 * w + ctz64(fm);
          int match = 0;
          if (lane() == 0)
            for (int f = tg(gf, TGM_FBEG); f < tg(gf, TGM_FEND) && !match; f++)
              match = rs_compatible(L, F, D.tg_frs + (int64_t)f * d.RSW, allow) ? 1 : 0;
          const bool keep = rdl(match, 0) != 0;
          mine = lane() == (gf & 63) ? (mine && keep) : mine;
        }
        const int v = mine ? tdom(g, node) : -1;
        if (v >= 0) tcnt_inc(tg(g, TGM_CNT) + v);  // recording registers the domain (distinct words per lane)
        const uint64_t hg = wballot(v >= 0 && tg(g, TGM_HOST) != 0);
        if (!SIM && logAt >= 0 && hg) W.log_hg[(int64_t)logAt * GMW + w] = hg;  // wave-wide store of a uniform value
      }
      hbm_release();
      wsync();
      return;
    }
    const uint64_t pres = rs_present(F), compl_ = rs_compl(F);
    for (int w = 0; w < GMW; w++) {
      uint64_t hg = 0;
      const uint64_t sel = gword(GS_SEL, w, t_sel), inv = gword(GS_INV, w, t_inv), act = gword(GS_ACT, w, t_active);
      for (uint64_t m = (sel & bits_below(d.G1, w) & act) | inv; m; m &= m - 1) {
        const int g = 64 * w + ctz64(m);
        const bool ownedGroup = g < d.G1;
        if (ownedGroup && tg(g, TGM_TYPE) == TG_SPREAD && tg(g, TGM_FEND) > tg(g, TGM_FBEG)) {  // nodeFilter
          int match = 0;
          if (lane() == 0)
            for (int f = tg(g, TGM_FBEG); f < tg(g, TGM_FEND) && !match; f++)
              match = rs_compatible(L, F, D.tg_frs + (int64_t)f * d.RSW, allow) ? 1 : 0;
          if (!rdl(match, 0)) continue;
        }
        if (node >= 0) {
          int rec = 0;
          if (lane() == 0) {
            const int v = tdom(g, node);
            if (v >= 0) tcnt_inc(tg(g, TGM_CNT) + v);  // recording registers the domain
            rec = v >= 0;
          }
          if (!SIM && tg(g, TGM_HOST) && rdl(rec, 0)) hg |= 1ull << (g & 63);
          continue;
        }
        const int k = tg(g, TGM_KEY), nv = tg(g, TGM_NV);
        if (!bit(pres, k)) continue;  // Get() of a missing key is Exists: no values
        const KeyMeta km = L.keys[k];
        if (ownedGroup && tg(g, TGM_TYPE) != TG_ANTI) {  // spread / affinity: only a collapsed domain
          int tot = 0;
          for (int wd = lane(); wd < km.nw; wd += kWave) tot += __popc(F[L.HDR + km.off + wd]);
          tot = wred_add(tot);
          if (bit(compl_, k) || tot != 1) continue;
        }
        bool any = false;
        for (int wd = lane(); wd < km.nw; wd += kWave) {  // anti-affinity: every domain of the requirement
          uint32_t x = F[L.HDR + km.off + wd];
          any = any || x != 0;
          while (x) {
            const int v = wd * 32 + __builtin_ctz(x);
            x &= x - 1;
            if (v >= nv) {
              if (claim >= 0) {  // -1: not registered in a late group (recording registers it)
                const int64_t at = (int64_t)g * W.ccs + claim;
                const int cc = W.tg_ccnt[at];
                W.tg_ccnt[at] = cc < 0 ? 1 : cc + 1;
                if (cc <= 0) W.tg_cpos[g] += 1;  // one more placeholder holding a counted pod
              }
            } else {
              tcnt_inc(tg(g, TGM_CNT) + v);
            }
          }
        }
        if (!SIM && tg(g, TGM_HOST) && wballot(any)) hg |= 1ull << (g & 63);
      }
      if (!SIM && logAt >= 0 && hg) W.log_hg[(int64_t)logAt * GMW + w] = hg;  // wave-wide store of a uniform value
    }
    hbm_release();
    wsync();
  }

  // Topology.Update for relaxation state s1 (topology.go:102-119), wave-wide: the late groups it owns that do not
  // exist yet are created now.  The NodeClaims made so far registered their placeholders before these groups
  // existed (NewNodeClaim's Register only reaches t.topologies), so their placeholder domains start unregistered.
  __device__ __forceinline__ void topo_activate_state(int s1, int nclaims, int hostCtr) {
    const int GMW = d.GMW;
    const uint64_t KS_G* own = D.st_gown + (int64_t)s1 * GMW;
    bool any = false;
    for (int w = 0; w < GMW; w++) {
      const uint64_t act = gword(GS_ACT, w, t_active), fresh = own[w] & ~act;
      if (!fresh) continue;
      any = true;
      for (uint64_t m = fresh; m; m &= m - 1) {
        const int g = 64 * w + ctz64(m);
        for (int c = lane(); c < nclaims; c += kWave) W.tg_ccnt[(int64_t)g * W.ccs + c] = -1;
        if (!SIM) W.tg_act[g] = hostCtr;  // placeholders up to this ordinal were never registered (uniform store)
      }
      if (w == 0) t_active = act | fresh;
      else s_gw[GS_ACT * GMW + w] = act | fresh;  // wave-wide store of a uniform value
    }
    if (any) hbm_release();
    wsync();
  }

  // --- NodeClaim quick reject at sorted position j: necessary conditions of NodeClaim.Add ------
  __device__ __forceinline__ bool claim_quick(int j, int s, int sflags, uint64_t toltpl, const int64_t* pod) const {
    if (!((toltpl >> s_ptpl[j]) & 1ull)) return false;  // Taints.Tolerates (nodeclaim.go:68-71)
    if (hpA() && (W.c_hp[s_order[j]] & cur_hpc)) return false;  // host port conflicts (:72-75)
    bool ok = true;
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      ok &= pod[r] <= s_phead[(int64_t)j * R() + r];
    }
    if (ok && keys(sflags))
      ok = rs_compatible(L, W.c_rs + (int64_t)s_order[j] * d.RSW, s_pin, d.allowWK);
    return ok;
  }

  // --- wave-cooperative NodeClaim.Add on claim c -------------------------------------------------
  // Builds s_rs / s_rem, the new requests, thresholds and option count.  Returns options left > 0.
  template <bool INL>
  __device__ __forceinline__ bool claim_full(int c, int s, int sflags, const int64_t* pod, int64_t* req, int* nthr,
                                             int& ncnt) {
    const ClaimView<INL>& v = cv<INL>();
    bool changed = false;
    PH_BEGIN(u0);
    if (keys(sflags) || (TOPO && t_any)) {
      const uint32_t KS_G* crs = W.c_rs + (int64_t)c * d.RSW;
      copy_words(s_rs, crs, d.RSW);
      wsync();
      if (keys(sflags))
        changed = rs_add_wave(L, s_rs, s_pin, (sflags & SF_TOUCHES_IT_KEYS) ? d.itKeys : 0);
      if (TOPO && t_any) {
        if (topo_apply(s_rs, c, d.allowWK) != 0) {  // topology requirements (nodeclaim.go:92-100)
          ncnt = 0;
          return false;
        }
        changed = !rs_equal_keys(L, s_rs, crs, d.itKeys);
      }
      algbytes += 8 * d.RSW;
    }
    const int t = tplv(uni(v.tpl[c]));
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      req[r] = v.req[(int64_t)c * R() + r] + pod[r];
      nthr[r] = uni(v.thr[(int64_t)c * R() + r]);
    }
    const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
    PHS_END(u0, 0);
    PH_BEGIN(u1);
    rem_same = false;
    if (!negR()) {
      // Requests only grow: the options a request no longer fits are a prefix of each resource's
      // Allocatable-ascending order beyond its threshold.
      int removed = 0, examined = 0;
      // the smallest Allocatable left beyond each resource's threshold, all read at once: a resource whose
      // request still fits it removes nothing and skips its ballot loop (the common step)
      int64_t nxt[RM];
      bool moves = false;
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= d.R) break;
        nxt[r] = nthr[r] < nIT ? tsort_a((int64_t)tb * R() + (int64_t)r * nIT + nthr[r]) : INT64_MAX;
        moves |= nxt[r] < req[r];
      }
      if (!changed && !moves) {  // the options stay as they are: no working copy, nothing to write back
        algbytes += 16 * R() + 4 * R();
        PHS_END(u1, 1);
        rem_same = true;
        ncnt = uni(v.cnt[c]);
        return ncnt > 0;
      }
      copy_words(s_rem, v.rem + (int64_t)c * d.TW, d.TW);
      wsync();
#ifdef KS_PHASE_STATS
      const uint64_t tmv = __builtin_amdgcn_s_memtime();
      kcyc[KD_THR_MOVES] += moves;
#endif
      [[maybe_unused]] bool more[RM] = {};  // KS_THR_BATCH: the resource's first chunk dropped all 64 (the loop below goes on from there)
      if constexpr (THR_BATCH) {
        // The resources' advances do not depend on each other: the clears commute and an option two resources drop
        // leaves the count once either way (the wave's LDS operations execute in order).  So the first chunk of every
        // resource goes out together, three LDS round trips in all instead of three per resource.  A lane with
        // nothing to drop reads the table's last entry and clears no bit (mask ~0); nIT > 0 here (moves or changed
        // with an option left).
        int pos[RM];
        bool ex[RM];
        uint32_t old[RM];
        thrBatchCalls++;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (RT == 0 && r >= d.R) break;
          const int i = nthr[r] + lane(), ii = i < nIT ? i : (nIT > 0 ? nIT - 1 : 0);
          const int64_t base = (int64_t)tb * R() + (int64_t)r * nIT;
          ex[r] = (nxt[r] < req[r]) & (i < nIT) & (tsort_a(base + ii) < req[r]);
          pos[r] = tsort_p(base + ii);
        }
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (RT == 0 && r >= d.R) break;
          const int q = ex[r] ? pos[r] : 0;
          old[r] = lds_and(s_rem + (q >> 5), ex[r] ? ~(1u << (q & 31)) : ~0u);
        }
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (RT == 0 && r >= d.R) break;
          const bool was = ex[r] & (((old[r] >> (pos[r] & 31)) & 1u) != 0);
          const int nm = __popcll(wballot(ex[r]));
          removed += __popcll(wballot(was));
          nthr[r] += nm;
          examined += nm;
          more[r] = nm == kWave;
        }
      }
      bool multi = false;  // some resource dropped options past its first chunk
      for (int r = 0; r < R(); r++) {
        const int64_t base = (int64_t)tb * R() + (int64_t)r * nIT;
        int k = nthr[r];
        if (THR_BATCH ? !more[r] : !(nxt[r] < req[r])) continue;
        while (k < nIT) {
          const int i = k + lane();
          const bool ex = i < nIT && tsort_a(base + i) < req[r];
          const uint64_t m = wballot(ex);
          if (m == 0) break;
          bool was = false;
          if (ex) {
            const int pos = tsort_p(base + i);
            const uint32_t bit = 1u << (pos & 31);
            was = (lds_and(s_rem + (pos >> 5), ~bit) & bit) != 0;
          }
          removed += __popcll(wballot(was));
          const int nm = __popcll(m);
          k += nm;
          examined += nm;
          if (nm < kWave) break;
        }
        if constexpr (THR_BATCH) multi |= k > nthr[r];
        nthr[r] = k;
      }
      if constexpr (THR_BATCH) thrMultiChunk += multi;
      algbytes += 8 * d.TW + 16 * R() + 4 * R() + (int64_t)examined * 12;
      wsync();
#ifdef KS_PHASE_STATS
      if (moves) kcyc[KD_CYC_THR_MOVE] += __builtin_amdgcn_s_memtime() - tmv;
#endif
      PHS_END(u1, 1);
      if (!changed) {
        ncnt = uni(v.cnt[c]) - removed;
        return ncnt > 0;
      }
      // Requirements changed: the options left are those the new requirements still admit, from
      // the feasibility masks (one word per lane), exact per position only for irregular ones.
      PH_BEGIN(u2);
      feas_masks(s_rs, t, fm_row(s, t));
      PHS_END(u2, 2);
      PH_BEGIN(u3);
      for (int w0 = 0; w0 < d.TW; w0 += kWave) {
        const int w = w0 + lane();
        uint32_t keep = 0, irr = 0;
        if (w < d.TW) {
          const uint32_t rem = s_rem[w];
          irr = rem & s_firr[w];
          keep = rem & ~s_firr[w] & s_fic[w] & s_fof[w];
        }
        for (uint64_t any = wballot(irr != 0); any; any &= any - 1) {  // rare: complement IT requirements
          const int ow = w0 + ctz64(any);
          const uint32_t bits = (uint32_t)rdl((int)irr, ow - w0);
          const bool mine = lane() < 32 && ((bits >> lane()) & 1u);
          bool ok = false;
          if (mine) {
            const int it = D.tpl_its[tb + ow * 32 + lane()];
            ok = rs_intersects(L, D.it_rs + (int64_t)it * d.RSW, s_rs) && has_offering(it, s_rs);
          }
          const uint32_t okb = (uint32_t)wballot(ok);
          if (w == ow) keep |= okb;
        }
        if (w < d.TW) s_rem[w] = keep;
      }
      wsync();
      ncnt = popc_words(s_rem, d.TW);
      algbytes += 12 * (int64_t)d.TW;
      PHS_END(u3, 3);
      return ncnt > 0;
    }
    copy_words(s_rem, v.rem + (int64_t)c * d.TW, d.TW);
    wsync();
    int cnt = 0, scanned = 0;
    if (changed) feas_masks(s_rs, t, fm_row(s, t));
    for (int base = 0; base < nIT; base += kWave) {
      const int wi = base >> 5;
      const uint64_t bits = (uint64_t)s_rem[wi] | (wi + 1 < d.TW ? (uint64_t)s_rem[wi + 1] << 32 : 0ull);
      uint64_t m = 0;
      if (bits) {
        const int gpos = tb + base + lane();
        const int pos = base + lane();
        bool ok = (bits >> lane()) & 1ull;
        if (ok) ok = fits_pos(req, gpos);
        if (ok && changed) {
          if (fbit(s_firr, pos)) {
            const int it = D.tpl_its[gpos];
            ok = rs_intersects(L, D.it_rs + (int64_t)it * d.RSW, s_rs) && has_offering(it, s_rs);
          } else {
            ok = fbit(s_fic, pos) && fbit(s_fof, pos);
          }
        }
        m = wballot(ok);
        scanned += __popcll(bits);
      }
      wsync();
      store_bits(s_rem, base, m);
      cnt += __popcll(m);
    }
    ncnt = cnt;
    algbytes += 8 * d.TW + 16 * R() + (int64_t)scanned * 8 * R();
    wsync();
    return cnt > 0;
  }

  // exact max Allocatable per resource over the options (quick-reject bound); refreshes the
  // headroom of the claim's sorted position `pos` (-1: none yet)
  template <bool INL, class PB>
  __device__ __forceinline__ void recompute_max(int c, PB bits, int t, int pos) {
    const ClaimView<INL>& v = cv<INL>();
    const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
    for (int r = 0; r < R(); r++) {
      int64_t m = INT64_MIN;
      if (!negR()) {  // the first option from the top of the Allocatable-ascending order
        const int64_t base = (int64_t)tb * R() + (int64_t)r * nIT;
        for (int k = nIT - 1; k >= 0; k -= kWave) {
          const int i = k - lane();
          bool in = false;
          if (i >= 0) {
            const int q = tsort_p(base + i);
            in = (bits[q >> 5] >> (q & 31)) & 1u;
          }
          const uint64_t hit = wballot(in);
          if (hit) {
            m = tsort_a(base + k - ctz64(hit));
            break;
          }
        }
      } else {
        for (int q = lane(); q < nIT; q += kWave)
          if ((bits[q >> 5] >> (q & 31)) & 1u) {
            const int64_t a = alloc_pos(tb + q, r);
            m = a > m ? a : m;
          }
        m = wred_max(m, (int64_t)INT64_MIN);
      }
      m = rdl64(m, 0);  // lane 0's value, stored by every lane (claim state is written wave-wide, see commit_claim)
      v.max[(int64_t)c * R() + r] = m;
      if (pos >= 0) s_phead[(int64_t)pos * R() + r] = m - v.req[(int64_t)c * R() + r];
    }
    if (!INL) hbm_release();
    wsync();
  }

  // Returns whether s.newNodeClaims is still non-decreasing after the increment at `pos`.
  template <bool INL>
  __device__ __forceinline__ bool commit_claim(int c, int pos, int n, int p, int sflags, const int64_t* pod,
                                               const int64_t* req, const int* nthr, int ncnt, int& nlog) {
    const ClaimView<INL>& v = cv<INL>();
    const int okNew = uni(s_okey[pos]) + 1;
    const bool srt = pos + 1 >= n || okNew <= uni(s_okey[pos + 1]);
    // Claim state is written by every lane with the same (wave-uniform) values rather than under
    // `lane() == 0`: a lane-0-only LDS store was lost in some builds, a wave-wide one has no
    // exec-mask region to get wrong.  Same-address stores of one value are benign.
    int64_t heads[RM];  // (each lane reads before it writes the same words: program order keeps it)
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      heads[r] = s_phead[(int64_t)pos * R() + r];
    }
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      v.req[(int64_t)c * R() + r] = req[r];
      v.thr[(int64_t)c * R() + r] = nthr[r];
      s_phead[(int64_t)pos * R() + r] = heads[r] - pod[r];
    }
    if constexpr (CAP_BOUND) {
      // The headroom now stored bounds Allocatable - requests of every option the claim has left (the quick test
      // rejects on it).  An identical pod above it in some resource fits none of them: run_cap gives 0 there for
      // every option, whatever the request (0, 1 or more).  A loose bound only leaves the call to be made.
      bool over = false;
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= d.R) break;
        over |= pod[r] > heads[r] - pod[r];
      }
      capOver = ub(over);
    }
    v.cnt[c] = ncnt;
    s_okey[pos] = okNew;
    if (hpA()) W.c_hp[c] |= cur_hpu;  // hostPortUsage.Add (wave-wide store of a uniform value)
    if (keys(sflags) || (TOPO && t_any)) copy_words(W.c_rs + (int64_t)c * d.RSW, s_rs, d.RSW);
    if (!rem_same) copy_words(v.rem + (int64_t)c * d.TW, s_rem, d.TW);
    log_commit(p, c, nlog);
    // The max bound stays valid as the options only shrink; it is tightened lazily when a full check
    // fails.  HBM-resident claim state is re-read by other lanes: drain the stores first.
    if (keys(sflags) || !INL || hpA()) hbm_release();
    wsync();
    if (TOPO && t_rec) {  // Topology.Record on the claim's final requirements (nodeclaim.go:121)
      if (keys(sflags) || t_any) topo_record(s_rs, c, -1, d.allowWK, nlog - 1);
      else topo_record(W.c_rs + (int64_t)c * d.RSW, c, -1, d.allowWK, nlog - 1);
    }
    algbytes += 24 * R() + 4 * d.TW + 8;
    return srt;
  }

  // --- runs of identical resource-only pods on one NodeClaim (LEAN Solve) -------------------------
  // After a pod lands on the claim at sorted position `pos` and s.newNodeClaims stays non-decreasing, an
  // identical next pod meets the same sort (nothing to reorder), the same rejections before `pos` (those
  // claims and the existing nodes did not change) and lands on this claim again while it accepts -- as
  // long as the claim's count stays <= the next position's.  The pods one claim takes that way: at most
  // M (the run, and that count bound), and at most as many as its best remaining option still fits:
  // max over the options of min over resources of floor((Allocatable - requests) / pod).
  template <bool INL>
  __device__ __forceinline__ int claim_run_cap(int c, const int64_t* pod, int M) const {
    const ClaimView<INL>& v = cv<INL>();
    const int tw = uni(v.tpl[c]), t = tplv(tw);
    const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
    float rq[RM];
    int64_t rc[RM];
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      rq[r] = run_rcp(pod[r]);
      rc[r] = v.req[(int64_t)c * R() + r];
    }
    int best = 0;
    if constexpr (RUN_FRONT && INL) {
      // The maximum is monotone in the Allocatable vector, so an option another remaining option dominates cannot
      // win.  A LEAN claim loses options through Fits alone, and whatever fits the dominated option fits the
      // dominating one: with every fitting front member among the claim's first options (TPL_FOK), each remaining
      // option has a remaining front member above it, and the maximum over those is the maximum.
      const int fb = s_fbeg[t], nf = s_fbeg[t + 1] - fb;  // at most kWave (pareto_fronts); 0: not pruned
      if ((tw & TPL_FOK) && nf > 0) {
        capFront++;
        const int q = lane() < nf ? s_front[fb + lane()] : 0;
        if (lane() < nf && ((v.rem[(int64_t)c * d.TW + (q >> 5)] >> (q & 31)) & 1u)) {
          int cap = M;
#pragma unroll
          for (int r = 0; r < RM; r++) {
            if (RT == 0 && r >= d.R) break;
            const int x = run_cap(alloc_pos(tb + q, r) - rc[r], pod[r], rq[r], M);
            cap = x < cap ? x : cap;
          }
          best = cap;
        }
        return wred_max(best, (int)0x80000000);
      }
    }
    capFull++;
    for (int q0 = 0; q0 < nIT; q0 += kWave) {
      const int q = q0 + lane();
      if (q < nIT && ((v.rem[(int64_t)c * d.TW + (q >> 5)] >> (q & 31)) & 1u)) {
        int cap = M;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (RT == 0 && r >= d.R) break;
          const int x = run_cap(alloc_pos(tb + q, r) - rc[r], pod[r], rq[r], M);
          cap = x < cap ? x : cap;
        }
        best = cap > best ? cap : best;
      }
    }
    return wred_max(best, (int)0x80000000);
  }
  // Commit of k identical pods (podk = k x pod, claim_full already applied to it) to claim c at sorted
  // position pos: commit_claim's stores with the count advanced by k.  Returns whether s.newNodeClaims
  // is still non-decreasing.
  template <bool INL>
  __device__ __forceinline__ bool commit_bulk(int c, int pos, int n, int k, const int64_t* podk, const int64_t* req,
                                              const int* nthr, int ncnt) {
    const ClaimView<INL>& v = cv<INL>();
    const int okNew = uni(s_okey[pos]) + k;
    const bool srt = pos + 1 >= n || okNew <= uni(s_okey[pos + 1]);
    int64_t heads[RM];
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= d.R) break;
      heads[r] = s_phead[(int64_t)pos * R() + r];
    }
#pragma unroll
    for (int r = 0; r < RM; r++) {  // wave-wide stores of uniform values (see commit_claim)
      if (RT == 0 && r >= d.R) break;
      v.req[(int64_t)c * R() + r] = req[r];
      v.thr[(int64_t)c * R() + r] = nthr[r];
      s_phead[(int64_t)pos * R() + r] = heads[r] - podk[r];
    }
    v.cnt[c] = ncnt;
    s_okey[pos] = okNew;
    if (!rem_same) copy_words(v.rem + (int64_t)c * d.TW, s_rem, d.TW);
    if (!INL) hbm_release();
    wsync();
    return srt;
  }

  // --- new NodeClaim from each template in order (scheduler.go:258-283) -----------------------
  // Returns 1 placed, 0 failed (fail codes recorded), 2 no templates (add() returns nil), -1 cap, -2 a record of
  // k_fresh_claims differs from the derivation (KS_TPL_TABLE_CHECK).
  __device__ __forceinline__ int try_templates(int p, int s, int sflags, uint64_t toltpl, const int64_t* pod,
                                               int& nclaims, int& nlog, int& hostCtr, bool& srt) {
    if (d.NTPL == 0) return 2;
    for (int t = 0; t < d.NTPL; t++) {
      uint32_t code = FC_NONE;
      int hostid = -1;
      const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
      const int pool = D.tpl_pool[t];
      PH_BEGIN(ttd);
      // KS_TPL_MEMO: without a NodePool limit the options, thresholds, option count and max Allocatable of a fresh
      // NodeClaim are a function of (t, pod): every instance type is a candidate, the requirements are the
      // template's (LEAN pods carry no keys and no topology), Fits tests tpl_daemon[t] + pod against static tables.
      // The state s -- one per pod, never shared -- enters only through k_feasibility's row (s, t), which a LEAN
      // problem does not have (fmOn needs a state with keys, KsDims::lean none; fm_row is then null for every s):
      // the memo is bypassed should the rows ever be on.  The last claim created that way is kept in LDS; an equal
      // key takes its values (it was created before, so it is no failure path) and runs everything else -- the
      // NewNodeClaim counter, the taint test, the claim cap, every store, the log, the algorithmic bytes.
      bool hit = false;
      if constexpr (TPL_MEMO) {
        if (pool < 0 && !d.fmOn) {
          hit = (int)s_memo[MM_T] == t;  // (uniform reads)
          const LI64 mp = (LI64)(s_memo + MM_POD);
          for (int r = 0; r < R(); r++) hit = hit && mp[r] == pod[r];
          hit = ub(hit);
        }
      }
      // KS_TPL_MASKS: under the same conditions the requirement and offering tests of every position are a function
      // of t alone -- every position is a candidate, the requirements are tpl_rs[t] -- and only Fits reads the pod.
      // The first derivation of t in this Solve keeps both bitsets (irregular positions resolved exactly); a later
      // miss reads them: no candidate loop, no feas_masks, no per-position requirement / offering test.  The three
      // booleans per position are the same, so the options, the failure flags and everything after are too.
      bool mk = false, mfill = false;
      if constexpr (TPL_MASKS) {
        if (pl.tmask && pool < 0 && !d.fmOn && !hit) {
          mk = uni((int)s_tmv[t]) != 0;
          mfill = !mk;
        }
      }
      const LU32 tm_ic = TPL_MASKS ? s_tmask + (int64_t)t * 2 * d.TW : s_tmask, tm_of = TPL_MASKS ? tm_ic + d.TW : s_tmask;
      // KS_TPL_TABLE: under the memo's conditions everything the memo keeps is a function of (t, the pod's requests),
      // and the handle holds it for every (request class, template): k_fresh_claims ran this derivation once, one
      // wave per pair.  A miss loads the pod's class and the record; a record with options becomes the memo's content
      // and the claim is created as on a hit (the memo then holds what the derivation would have left in it, so its
      // later hits are the same ones).  A record without options takes the derivation, which sets the failure flags.
      bool tabTry = false, tab = false;
      const uint32_t KS_G* chk = nullptr;  // KS_TPL_TABLE_CHECK: the record to compare the derivation with
      if constexpr (TPL_TABLE) tabTry = pool < 0 && !d.fmOn && !hit;
      // filterByRemainingResources (scheduler.go:364-383)
      uint64_t anyCand = 0;
      for (int base = 0; base < (hit || mk || tabTry ? 0 : nIT); base += kWave) {  // (tabTry: no limit, all candidates)
        const int pos = base + lane();
        bool ok = pos < nIT;
        if (ok && pool >= 0) {
          const uint32_t mask = D.pool_mask[pool];
          const int64_t KS_G* cap = D.it_cap + (int64_t)D.tpl_its[tb + pos] * R();
          for (int r = 0; r < R(); r++)
            if (((mask >> r) & 1u) && cap[r] > s_pool[(int64_t)pool * R() + r]) ok = false;
        }
        const uint64_t m = wballot(ok);
        store_bits(s_cand, base, m);
        anyCand |= m;
      }
      wsync();
      YPH_END(ttd, YS_TPL_CAND);
      if (pool >= 0 && anyCand == 0) {
        code = FC_LIMITS;
      } else {
        hostid = ++hostCtr;  // NewNodeClaim: atomic.AddInt64(&nodeID, 1) (nodeclaim.go:48)
        if (!((toltpl >> t) & 1ull)) {
          code = FC_TAINTS;
        } else {
          PH_BEGIN(tyc);
          copy_words(s_rs, D.tpl_rs + (int64_t)t * d.RSW, d.RSW);
          wsync();
          YPH_END(tyc, YS_TPL_CAND);
          bool ok = true;
          if (keys(sflags)) {
            ok = rs_compatible(L, s_rs, s_pin, d.allowWK);
            if (ok) rs_add_wave(L, s_rs, s_pin, 0);
          }
          if (TOPO && ok && t_any) {  // topology requirements of the fresh NodeClaim (nodeclaim.go:92-100)
            const uint32_t tc = topo_apply(s_rs, nclaims, d.allowWK);
            if (tc) {
              ok = false;
              code = tc;
              const int64_t slot = ((int64_t)p * d.NTPL + t) * d.FSW;
              if (SIM) {  // simulations render no messages
              } else if (tc == FC_TOPO_COMPAT) {
                copy_words(W.fail_rs + slot, s_rs, d.RSW);  // the topology requirements, for the message
              } else {
                const int g = (int)(tc >> 16) & 0xffff, nv = tg(g, TGM_NV);
                if (!tg(g, TGM_HOST))  // the counts (-1: unregistered), for the message (FSW fits them)
                  for (int v = lane(); v < nv; v += kWave) W.fail_rs[slot + v] = (uint32_t)tcnt(g, v);
                else if (lane() == 0)  // hostname: the commits so far; the host replays their log_hg entries
                  W.fail_rs[slot] = (uint32_t)nlog;
              }
            }
          }
          if (!ok) {
            if (code == FC_NONE) code = FC_COMPAT;
          } else {
            int64_t req[RM];
            for (int r = 0; r < R(); r++) req[r] = D.tpl_daemon[(int64_t)t * R() + r] + pod[r];
            uint32_t flags = 0;
            uint64_t any = 0;
            if constexpr (TPL_TABLE) {
              if (tabTry) {
                const int nw = tpl_memo_words(R(), d.TW);
                // the block: pod_class, then the table (ks_problem.h).  Class -1: this handle has no table
                const int32_t KS_G* blk = D.tpl_front + tpl_block_base(D.frontTotal);
                const int cls = uni(blk[p]);
                const uint32_t KS_G* rec = (const uint32_t KS_G*)blk + tpl_block_table(d.P) + ((int64_t)(cls < 0 ? 0 : cls) * d.NTPL + t) * nw;
                const uint32_t v0 = cls >= 0 && lane() < nw ? rec[lane()] : 0u;  // one lane per word
                if (rdl((int)v0, MM_CNT) > 0) {
                  tableHits.n++;
                  if constexpr (TPL_TABLE_CHECK) {
                    chk = rec;
                  } else {
                    if (lane() < nw) s_memo[lane()] = v0;
                    for (int i = kWave + lane(); i < nw; i += kWave) s_memo[i] = rec[i];
                    wsync();
                    hit = tab = true;
                  }
                }
              }
            }
            if (hit) {  // the memo's options
              copy_words(s_rem, s_memo + MM_POD + 5 * R(), d.TW);
              any = 1;
            } else if (!mk) {
              PH_BEGIN(tyf);
              feas_masks(s_rs, t, fm_row(s, t));
              YPH_END(tyf, YS_TPL_FEAS);
            }
            PH_BEGIN(tyl);
            for (int base = 0; base < (hit ? 0 : nIT); base += kWave) {
              const int pos = base + lane();
              const bool in = pos < nIT && (mk || tabTry || ((s_cand[pos >> 5] >> (pos & 31)) & 1u));
              bool ic = false, fi = false, of = false;
              if (in) {
                if (mk) {
                  ic = fbit(tm_ic, pos);
                  of = fbit(tm_of, pos);
                } else if (fbit(s_firr, pos)) {
                  const int it = D.tpl_its[tb + pos];
                  ic = rs_intersects(L, D.it_rs + (int64_t)it * d.RSW, s_rs);
                  of = has_offering(it, s_rs);
                } else {
                  ic = fbit(s_fic, pos);
                  of = fbit(s_fof, pos);
                }
                fi = fits_pos(req, tb + pos);
              }
              if (wballot(ic)) flags |= FF_REQ;
              if (wballot(fi)) flags |= FF_FITS;
              if (wballot(of)) flags |= FF_OFF;
              if (wballot(ic && fi && !of)) flags |= FF_REQ_FITS;
              if (wballot(ic && of && !fi)) flags |= FF_REQ_OFF;
              if (wballot(fi && of && !ic)) flags |= FF_FITS_OFF;
              const uint64_t m = wballot(ic && fi && of);
              store_bits(s_rem, base, m);
              any |= m;
              if constexpr (TPL_MASKS) {
                if (mfill) {
                  store_bits(tm_ic, base, wballot(ic));
                  store_bits(tm_of, base, wballot(of));
                }
              }
            }
            if constexpr (TPL_MASKS) {
              if (mfill) {
                s_tmv[t] = 1u;  // wave-wide store of a uniform value
                maskFills++;
              }
            }
            algbytes += 4 * d.RSW + (int64_t)nIT * (8 * R() + 4 * d.RSW + 16);
            wsync();
            YPH_END(tyl, YS_TPL_FILTER);
            if (any == 0) {
              code = FC_NO_IT | (flags << 8);
              if (!SIM && TOPO && t_any) {  // the message prints the requirements the topology narrowed
                copy_words(W.fail_rs + ((int64_t)p * d.NTPL + t) * d.FSW, s_rs, d.RSW);
                code |= FC_RS_SNAP;
              }
            } else {
              if (nclaims >= pl.KO) return -1;
              const int c = nclaims++;
              XPH_END(ttd, SS_TPL_DERIVE);
              PH_BEGIN(tts0);
              if (SIM && TOPO)  // the next fresh claim's placeholder counts (a simulation zeroes one column per claim)
                for (int g = lane(); g < d.G; g += kWave) W.tg_ccnt[(int64_t)g * W.ccs + nclaims] = 0;
              const bool inl = c < pl.KL;
              copy_words(W.c_rs + (int64_t)c * d.RSW, s_rs, d.RSW);
              if (inl) copy_words(lc.rem + (int64_t)c * d.TW, s_rem, d.TW);
              else copy_words(gc.rem + (int64_t)c * d.TW, s_rem, d.TW);
              XPH_END(tts0, SS_TPL_STORE);
              PH_BEGIN(ttd1);
              // thresholds: how much of each resource's ascending Allocatable order req excludes
              int thr[RM];
              for (int r = 0; r < R(); r++) {
                if (hit) {
                  thr[r] = uni((int)s_memo[MM_POD + 4 * R() + r]);
                  continue;
                }
                const int64_t b = (int64_t)tb * R() + (int64_t)r * nIT;
                int k = 0;
                for (int q = 0; q < nIT; q += kWave)
                  k += __popcll(wballot(q + lane() < nIT && tsort_a(b + q + lane()) < req[r]));
                thr[r] = k;
              }
              const int cnt = hit ? uni((int)s_memo[MM_CNT]) : popc_words(s_rem, d.TW);
              // KS_RUN_FRONT: did requirements, offerings or a NodePool limit keep a front member that Fits out
              // of the options?  (claim_run_cap then scans every option of this claim)
              bool fok = false;
              if constexpr (RUN_FRONT) {
                if (hit) {
                  fok = uni((int)s_memo[MM_FOK]) != 0;
                } else {
                  const int fb = s_fbeg[t], nf = s_fbeg[t + 1] - fb;
                  const int q = lane() < nf ? s_front[fb + lane()] : 0;
                  const bool miss = lane() < nf && fits_pos(req, tb + q) && !((s_rem[q >> 5] >> (q & 31)) & 1u);
                  fok = nf > 0 && wballot(miss) == 0;
                }
              }
              XPH_END(ttd1, SS_TPL_DERIVE);
              YPH_END(ttd1, YS_TPL_THR);
              PH_BEGIN(tts1);
              // wave-wide stores of uniform values (see commit_claim)
              for (int r = 0; r < R(); r++) {
                if (inl) {
                  lc.req[(int64_t)c * R() + r] = req[r];
                  lc.thr[(int64_t)c * R() + r] = thr[r];
                } else {
                  gc.req[(int64_t)c * R() + r] = req[r];
                  gc.thr[(int64_t)c * R() + r] = thr[r];
                }
              }
              if (inl) {
                lc.tpl[c] = RUN_FRONT && fok ? t | (int)TPL_FOK : t;
                lc.cnt[c] = cnt;
              } else {
                gc.cnt[c] = cnt;
              }
              W.c_tpl[c] = t;  // wave-wide stores of uniform values (see commit_claim)
              W.c_hp[c] = cur_hpu;
              W.c_host[c] = hostid;
              s_order[c] = c;
              s_okey[c] = 1;
              s_ptpl[c] = t;
              srt = c == 0 || uni(s_okey[c - 1]) <= 1;
              log_commit(p, c, nlog);
              hbm_release();  // c_rs / c_tpl / overflow state are read by other lanes later
              wsync();
              XPH_END(tts1, SS_TPL_STORE);
              if (TOPO && t_rec) topo_record(s_rs, c, -1, d.allowWK, nlog - 1);
              PH_BEGIN(ttm);
              if (hit) {  // recompute_max's stores with the memo's values
                const LI64 mx = (LI64)(s_memo + MM_POD + 2 * R());
                for (int r = 0; r < R(); r++) {
                  const int64_t m = uni64(mx[r]);
                  if (inl) lc.max[(int64_t)c * R() + r] = m;
                  else gc.max[(int64_t)c * R() + r] = m;
                  s_phead[(int64_t)c * R() + r] = m - req[r];
                }
                if (!inl) hbm_release();
                wsync();
                if (!tab) memoHits++;
              } else {
                if (mk) maskHits++;
                if (inl) recompute_max<true>(c, s_rem, t, c);
                else recompute_max<false>(c, s_rem, t, c);
                if constexpr (TPL_MEMO) {
                  if (pool < 0 && !d.fmOn) {  // keep what this claim derived (wave-wide stores of uniform values)
                    const LI64 mp = (LI64)(s_memo + MM_POD);
                    for (int r = 0; r < R(); r++) {
                      mp[r] = pod[r];
                      mp[R() + r] = inl ? uni64(lc.max[(int64_t)c * R() + r]) : uni64(ld_sc1(gc.max + (int64_t)c * R() + r));
                      s_memo[MM_POD + 4 * R() + r] = (uint32_t)thr[r];
                    }
                    copy_words(s_memo + MM_POD + 5 * R(), s_rem, d.TW);
                    s_memo[MM_T] = (uint32_t)t;
                    s_memo[MM_CNT] = (uint32_t)cnt;
                    if constexpr (RUN_FRONT) s_memo[MM_FOK] = fok ? 1u : 0u;
                    wsync();
                    if constexpr (TPL_TABLE_CHECK) {
                      if (chk) {  // every word the derivation left in the memo against the record's (word 3 and the R
                                  // words behind the options are padding)
                        // (the first differing word goes to the host in the masks' counters, which the table's
                        // build leaves unused: KS_TPL_MASKS is off with it)
                        int bi = -1;
                        uint32_t bd = 0, br = 0;
                        for (int i = lane(); i < MM_POD + 5 * R() + d.TW; i += kWave)
                          if (bi < 0 && i != 3 && s_memo[i] != chk[i]) {
                            bi = i;
                            bd = s_memo[i];
                            br = chk[i];
                          }
                        if (const uint64_t bm = wballot(bi >= 0)) {
                          const int l = ctz64(bm);
                          maskFills = rdl(bi, l);
                          maskHits = (int64_t)(((uint64_t)(uint32_t)rdl((int)bd, l) << 32) | (uint32_t)rdl((int)br, l));
                          return -2;
                        }
                      }
                    }
                  }
                }
              }
              XPH_END(ttm, SS_TPL_MAX);
              if (pool >= 0) {  // subtractMax (scheduler.go:347-362)
                const uint32_t mask = D.pool_mask[pool];
                for (int r = 0; r < R(); r++) {
                  if (!((mask >> r) & 1u)) continue;
                  int64_t m = INT64_MIN;
                  for (int pos = lane(); pos < nIT; pos += kWave)
                    if ((s_rem[pos >> 5] >> (pos & 31)) & 1u) {
                      const int64_t v = D.it_cap[(int64_t)D.tpl_its[tb + pos] * R() + r];
                      m = v > m ? v : m;
                    }
                  m = wred_max(m, (int64_t)INT64_MIN);
                  s_pool[(int64_t)pool * R() + r] -= m;  // wave-wide (m is reduced over the wave)
                }
                wsync();
              }
              return 1;
            }
          }
        }
      }
      W.fail_code[(int64_t)p * d.NTPL + t] = code;  // wave-wide stores of uniform values
      W.fail_host[(int64_t)p * d.NTPL + t] = hostid;
    }
    return 0;
  }

  // k_fresh_claims: what try_templates' derivation leaves in s_memo for a fresh NodeClaim of template t (no NodePool
  // limit, no feasibility rows) and a pod with these requests -- every position a candidate, the template's own
  // requirement record in s_rs, the same feas_masks / irregular-position tests, Fits of tpl_daemon[t] + pod, the
  // threshold counts, the front test and recompute_max, written through lc.max.  No option left: count 0 and the key.
  __device__ __forceinline__ void fresh_record(int t, const int64_t* pod) {
    const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
    int64_t req[RM];
    for (int r = 0; r < R(); r++) req[r] = D.tpl_daemon[(int64_t)t * R() + r] + pod[r];
    for (int i = lane(); i < tpl_memo_words(R(), d.TW); i += kWave) s_memo[i] = 0;
    for (int i = lane(); i < d.TW; i += kWave) s_rem[i] = 0;
    copy_words(s_rs, D.tpl_rs + (int64_t)t * d.RSW, d.RSW);
    wsync();
    feas_masks(s_rs, t);
    for (int base = 0; base < nIT; base += kWave) {
      const int pos = base + lane();
      bool ic = false, fi = false, of = false;
      if (pos < nIT) {
        if (fbit(s_firr, pos)) {
          const int it = D.tpl_its[tb + pos];
          ic = rs_intersects(L, D.it_rs + (int64_t)it * d.RSW, s_rs);
          of = has_offering(it, s_rs);
        } else {
          ic = fbit(s_fic, pos);
          of = fbit(s_fof, pos);
        }
        fi = fits_pos(req, tb + pos);
      }
      store_bits(s_rem, base, wballot(ic && fi && of));
    }
    wsync();
    const int cnt = popc_words(s_rem, d.TW);
    const LI64 mp = (LI64)(s_memo + MM_POD);
    for (int r = 0; r < R(); r++) mp[r] = pod[r];  // wave-wide stores of uniform values (see commit_claim)
    s_memo[MM_T] = (uint32_t)t;
    s_memo[MM_CNT] = (uint32_t)cnt;
    if (cnt > 0) {
      for (int r = 0; r < R(); r++) {
        const int64_t b = (int64_t)tb * R() + (int64_t)r * nIT;
        int k = 0;
        for (int q = 0; q < nIT; q += kWave)
          k += __popcll(wballot(q + lane() < nIT && tsort_a(b + q + lane()) < req[r]));
        s_memo[MM_POD + 4 * R() + r] = (uint32_t)k;
      }
      const int fb = s_fbeg[t], nf = s_fbeg[t + 1] - fb;
      const int q = lane() < nf ? s_front[fb + lane()] : 0;
      const bool miss = lane() < nf && fits_pos(req, tb + q) && !((s_rem[q >> 5] >> (q & 31)) & 1u);
      s_memo[MM_FOK] = nf > 0 && wballot(miss) == 0 ? 1u : 0u;
      copy_words(s_memo + MM_POD + 5 * R(), s_rem, d.TW);
      lc.max = mp + R();  // claim 0's max Allocatable is the record's
      recompute_max<true>(0, s_rem, t, -1);
    }
    wsync();
  }

  // try_templates' NewNodeClaim calls for a pod every template fails on topology (simNoClaim): a template whose
  // instance types all exceed its NodePool's remaining limits fails before NewNodeClaim (scheduler.go:262-268);
  // every other one increments the hostname counter (nodeclaim.go:44-48).  Returns 0 (the pod is not placed).
  __device__ __forceinline__ int sim_template_calls(int& hostCtr) const {
    for (int t = 0; t < d.NTPL; t++) {
      const int pool = D.tpl_pool[t];
      bool call = pool < 0;
      if (!call) {
        const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
        const uint32_t mask = D.pool_mask[pool];
        uint64_t anyCand = 0;
        for (int base = 0; base < nIT && !anyCand; base += kWave) {
          const int pos = base + lane();
          bool ok = pos < nIT;
          if (ok) {
            const int64_t KS_G* cap = D.it_cap + (int64_t)D.tpl_its[tb + pos] * R();
            for (int r = 0; r < R(); r++)
              ok = ok && !(((mask >> r) & 1u) && cap[r] > s_pool[(int64_t)pool * R() + r]);
          }
          anyCand = wballot(ok);
        }
        call = anyCand != 0;
      }
      if (call) hostCtr = uni(hostCtr + 1);
    }
    return 0;
  }

  // Returns how it was done: SORT_FAST (the wave-parallel partialInsertionSort finished it), SORT_EXACT (the
  // exact pdqsort ran) or SORT_CLOSED.  `pos`: the sorted position whose count increment left the descent, -1
  // when it has another origin (an appended claim) -- used only where the closed form is compiled in
  // (KS_SORT_CLOSED); `npos`: where that claim went (SORT_CLOSED), else -1.
  enum : int { SORT_FAST = 0, SORT_EXACT = 1, SORT_CLOSED_FORM = 2 };
  static constexpr bool SORT_CLOSED = !SIM && (KS_SORT_CLOSED == 2 || (KS_SORT_CLOSED == 1 && LEAN));
  // (the LEAN Solve alone: its resource count is a compile-time 3 or 4, which the shift keeps in registers)
  static constexpr bool CLOSED_SHIFT = KS_CLOSED_SHIFT && SORT_CLOSED && LEAN && RT > 0;
  // the general re-sort's register copy (KS_SORT_REGS: the LEAN Solve's out-of-line claim_sort_general_out)
  static constexpr bool SORT_REGS = KS_SORT_REGS != 0 && KS_SORT_OUTLINE && LEAN && !SIM;
  int sortsRegs = 0, sortRegsOver = 0, sortRegsBail = 0;  // general re-sorts finished from registers / too large for
                                                          // the copy / abandoned on a failed invariant (0)
  int64_t shiftDiff = 0;  // diagnostic build: moved entries whose shifted s_ptpl / s_phead differ from a regather
  // the top frame's hint and pivot from n and pos alone (KS_PIVOT_ARITH; the LEAN Solve, where pos is tracked)
  static constexpr bool PIVOT_ARITH = KS_PIVOT_ARITH && SORT_CLOSED && LEAN;
  // (their counters are members of the LEAN Solve alone: the other instantiations' Solver keeps its layout)
  struct ResortCtr {
    int cross50 = 0, arith = 0;        // re-sorts with pos >= 0 and n >= 50 / those decided without samples
    int append50 = 0, appClosed = 0;   // appended-claim re-sorts with n >= 50 / those taken by the closed form
    int64_t diff = 0;  // diagnostic build (KS_PIVOT_ARITH_CHECK): re-sorts whose sampled hint or pivot differs
  };
  struct NoResortCtr {};
  static constexpr bool RESORT_CTR = SORT_CLOSED && LEAN;
  [[no_unique_address]] std::conditional_t<RESORT_CTR, ResortCtr, NoResortCtr> rsc;
  // the appended claim's re-sort by its closed form (KS_APPEND_CLOSED; the shift keeps R resources in registers)
  static constexpr bool APPEND_CLOSED = KS_APPEND_CLOSED && SORT_CLOSED && LEAN && RT > 0;
  // `app`: the descent is an appended claim's (try_templates left it; pos is -1)
  __device__ __forceinline__ int sort_claims(int n, int pos, int& npos, bool app = false) {
    int tlo = n, thi = -1, pivot = -1;
    bool done = false;
    PH_BEGIN(tsc);
#ifdef KS_PHASE_STATS
    if (n <= 12) XPH_COUNT(SS_SORTS_LE12);
    else if (n < 50) XPH_COUNT(SS_SORTS_LT50);
#endif
    bool closed = false, shifted = false, appc = false;
    npos = -1;
    if constexpr (RESORT_CTR) rsc.append50 += app && n >= 50 ? 1 : 0;
    if constexpr (APPEND_CLOSED) {
      if (app && n >= 50) {
        const int p = append_closed<RM>(n, s_ptpl, s_phead);
        if (p >= 0) {  // SORT_FAST with partialInsertionSort's span; the four arrays moved: nothing to regather
          tlo = p;
          thi = n - 1;
          done = shifted = appc = true;
          rsc.appClosed++;
        }
      }
    }
    if (n > 12 && !appc) {  // pdqsort_func's top-level frame: choosePivot (reads only), then partialInsertionSort
      int hint = 0, pv = 0, ts = -1;
      if constexpr (RESORT_CTR) rsc.cross50 += pos >= 0 && n >= 50 ? 1 : 0;
#if KS_PIVOT_ARITH_CHECK
      if constexpr (RESORT_CTR) {  // both forms, on the array as the re-sort meets it
        if (pos >= 0 && n >= 50 && pos + 1 < n && ub(s_okey[pos] > s_okey[pos + 1])) {
          int hs = 0;
          const int ps = w_choose_pivot(0, n, hs);
          const bool off = !pivot_sampled(n, pos);
          rsc.diff += (hs == 1) != off || (off && ps != n / 4 * 2) ? 1 : 0;
        }
      }
#endif
      if constexpr (CLOSED_SHIFT) {
        bool arith = false;
        ts = closed_crossing<RM, PIVOT_ARITH>(n, pos, s_ptpl, s_phead, hint, pv, arith);
        rsc.arith += arith ? 1 : 0;
      } else if constexpr (PIVOT_ARITH) {
        // the hint by arithmetic: closed_move confirms the descent (-1: the samples, as before)
        int t = -1;
        if (pos >= 0 && n >= 50 && pos + 1 < n && !pivot_sampled(n, pos)) t = closed_move(n, pos);
        if (t >= 0) {
          pivot = n / 4 * 2;
          tlo = pos;
          thi = npos = pos + t;
          done = closed = true;
          rsc.arith++;
        } else {
          PH_BEGIN(tpv);
          pv = w_choose_pivot(0, n, hint);
          ZPH_END(tpv, ZS_PIVOT);
        }
      } else {
        PH_BEGIN(tpv);
        pv = w_choose_pivot(0, n, hint);
        ZPH_END(tpv, ZS_PIVOT);
      }
      if (hint == 1) {
        pivot = pv;
        if (ts >= 0) {  // s_ptpl and s_phead moved with their claims: nothing to regather
          tlo = pos;
          thi = npos = pos + ts;
          done = closed = shifted = true;
        }
        // (with the arithmetic hint this cannot succeed: off the sample positions closed_move has run and found no
        // descent at pos, on them a descent at pos makes the sampled hint something else)
        if constexpr (SORT_CLOSED && !CLOSED_SHIFT && !PIVOT_ARITH) {
          if (pos >= 0 && n >= 50 && pos + 1 < n) {
            const int t = closed_move(n, pos);
            if (t >= 0) {
              tlo = pos;
              thi = npos = pos + t;
              done = closed = true;
            }
          }
        }
      }
    }
    if (!closed && !appc) {
      // (out of line in the LEAN Solve, whose closed form leaves this the rare path; the other instantiations
      // keep it inlined, as measured before)
      const uint32_t g = KS_SORT_OUTLINE && LEAN && !SIM ? claim_sort_general_out(s_okey, s_order, n, pivot)
                                                          : claim_sort_general<LEAN && !SIM>(s_okey, s_order, n, pivot);
      tlo = (int)(g & 0x7fff);
      thi = (int)(g >> 15 & 0x7fff) - 1;
      done = g >> 30 & 1;
      if constexpr (SORT_REGS) {  // more claims than the copy holds is expected; any other refusal is a bug signal
        const bool over = n > (KS_SORT_REGS_N64 ? 64 : kSortRegsMax);
        sortsRegs += (int)(g >> 31);
        sortRegsOver += over ? 1 : 0;
        sortRegsBail += !over && !(g >> 31) ? 1 : 0;
      }
    }
    wsync();
#ifdef KS_PHASE_STATS
    if (shifted) {  // the invariant the shift rests on: what it moved is what the regather would have written
      int diff = 0;
      for (int j = tlo + lane(); j <= thi; j += kWave) {
        const int c = s_order[j];
        const bool inl = c < pl.KL;
        bool ne = s_ptpl[j] != (inl ? tplv(lc.tpl[c]) : W.c_tpl[c]);
        for (int r = 0; r < R(); r++) {
          const int64_t i = (int64_t)c * R() + r;
          ne = ne || s_phead[(int64_t)j * R() + r] != (inl ? lc.max[i] - lc.req[i] : gc.max[i] - gc.req[i]);
        }
        diff += ne ? 1 : 0;
      }
      shiftDiff += wred_add(diff);
    }
#endif
    if (!shifted) {
      PH_BEGIN(trg);
      for (int j = tlo + lane(); j <= thi; j += kWave) {
        const int c = s_order[j];
        const bool inl = c < pl.KL;
        s_ptpl[j] = inl ? tplv(lc.tpl[c]) : W.c_tpl[c];
        for (int r = 0; r < R(); r++) {
          const int64_t i = (int64_t)c * R() + r;
          s_phead[(int64_t)j * R() + r] = inl ? lc.max[i] - lc.req[i] : gc.max[i] - gc.req[i];
        }
      }
      wsync();
      ZPH_END(trg, ZS_REGATHER);
    }
    algbytes += (int64_t)(thi - tlo + 1) * (8 + 16 * R());
#ifdef KS_PHASE_STATS
    if (closed) XPH_END(tsc, SS_SORT_CLOSED);
    else if (done) XPH_END(tsc, SS_SORT_FAST);
    else {
      XPH_END(tsc, SS_SORT_EXACT);
      const uint64_t dt = __builtin_amdgcn_s_memtime() - tsc;
      ecyc[0] += n <= 12 ? dt : 0;
      ecyc[1] += n > 12 && n < 50 ? dt : 0;
      ecyc[2] += n >= 50 ? dt : 0;
    }
#endif
    return closed ? SORT_CLOSED_FORM : done ? SORT_FAST : SORT_EXACT;
  }

  // --- a run's deferred move (KS_RUN_FUSE, ks_solve_body.inc) --------------------------------------
  // Each closed-form crossing of a run lifts its claim over the block of entries below its count and changes
  // nothing else, so a run's crossings compose into one shift: the position arrays stay as they are while the
  // run advances, and the claim's entry (physically at pos0) is moved to its position p with count K once.
  // The entries after p below K: the first t of them, the array being sorted there (sort_claims' count).
  __device__ __forceinline__ int run_count_below(int p, int n, int K) const {
    int t = 0;
    for (int base = p + 1; base < n; base += 4 * kWave) {
      uint64_t m[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int q = base + u * kWave + lane();
        m[u] = wballot(q < n && s_okey[q] < K);
      }
      bool end = false;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        t += end ? 0 : popc64(m[u]);
        end = end || m[u] != ~0ull;
      }
      if (end) break;
    }
    return t;
  }
  // The move itself, the count, and sort_claims' regather of s_ptpl / s_phead over the positions it changed.
  __device__ __forceinline__ void run_materialise(int pos0, int p, int K) {
    pis_move(pos0, p);
    s_okey[p] = K;  // wave-wide store of a uniform value
    wsync();
    if (p == pos0) return;
    for (int j = pos0 + lane(); j <= p; j += kWave) {
      const int c = s_order[j];
      const bool inl = c < pl.KL;
      s_ptpl[j] = inl ? tplv(lc.tpl[c]) : W.c_tpl[c];
      for (int r = 0; r < R(); r++) {
        const int64_t i = (int64_t)c * R() + r;
        s_phead[(int64_t)j * R() + r] = inl ? lc.max[i] - lc.req[i] : gc.max[i] - gc.req[i];
      }
    }
    wsync();
  }

  // --- consolidation decision for this simulation (SIM epilogue) -------------------------------
  // worstLaunchPrice (helpers.go:235-258): the max price over the available offerings of the
  // preferred capacity type (spot first) whose zone the requirements allow.
  template <class PR>
  __device__ __forceinline__ double worst_price(int it, PR rs, bool spot, bool od) const {
    const int b = D.it_off_beg[it], e = D.it_off_beg[it + 1];
    for (int pass = 0; pass < 2; pass++) {
      if (!(pass == 0 ? spot : od)) continue;
      const int want = pass == 0 ? d.spotBit : d.odBit;
      bool any = false;
      double w = 0;
      for (int o = b; o < e; o++)
        if (D.off_ct[o] == want && rs_member(L, rs, d.zoneKey, D.off_zone[o])) {
          const double pr = D.off_price[o];
          if (!any || pr > w) w = pr;
          any = true;
        }
      if (any) return w;
    }
    return __DBL_MAX__;
  }
  // filterByPrice (helpers.go:160-169) over the options bitset `in` of template t -> `out`
  template <class PI, class PO, class PR>
  __device__ __forceinline__ int price_filter(PI in, PO out, int t, PR rs, bool spot, bool od, double price) const {
    const int tb = s_tbeg[t], nIT = s_tbeg[t + 1] - tb;
    int cnt = 0;
    for (int base = 0; base < nIT; base += kWave) {
      const int pos = base + lane();
      bool keep = pos < nIT && ((in[pos >> 5] >> (pos & 31)) & 1u);
      if (keep) keep = worst_price(D.tpl_its[tb + pos], rs, spot, od) < price;
      const uint64_t m = wballot(keep);
      if (lane() == 0) {
        out[base >> 5] = (uint32_t)m;
        if ((base >> 5) + 1 < d.TW) out[(base >> 5) + 1] = (uint32_t)(m >> 32);
      }
      cnt += __popcll(m);
    }
    return cnt;
  }
  // simulateScheduling's post-check (helpers.go:115-124) + computeConsolidation (consolidation.go:
  // 113-194) + filterOutSameType (multinodeconsolidation.go:155-188), into the record W.rec
  // anyPushed: some pod failed an attempt (its status array exists, sim_queue_init); otherwise every pod was placed.
  __device__ __forceinline__ void sim_record(int P, int nclaims, int hostCtr, bool allSched, int err, bool anyPushed,
                                             bool anyRelaxed) {
    if (anyPushed) {
      hbm_release();  // pod statuses written by lane 0
      bool bad = false;
      for (int i = lane(); i < P; i += kWave)
        bad |= ld_sc1(W.pod_status + i) == ST_FAILED && !(D.pod_flags[W.pod_map[i]] & PF_PROVISIONABLE);
      allSched = allSched && wballot(bad) == 0;
    }
    int32_t KS_G* rec = W.rec;
    const int TW = d.TW;
    int32_t KS_G* o_opt = rec + RF_HDR;
    int32_t KS_G* o_price = o_opt + TW;
    int32_t KS_G* o_same = o_price + TW;
    for (int i = lane(); i < 3 * TW; i += kWave) o_opt[i] = 0;
    int flags = (allSched ? RB_ALL_SCHEDULED : 0) | (anyRelaxed ? RB_RELAXED : 0), tpl = -1, host = -1, nopt = 0,
        nprice = 0, nsame = 0;
    int action = CA_NOOP;
    if (nclaims > 0 && err == KE_OK) {
      const int c = uni(s_order[0]);
      const bool inl = c < pl.KL;
      tpl = inl ? tplv(uni(lc.tpl[c])) : uni(W.c_tpl[c]);
      host = W.c_host[c];
      const uint32_t KS_G* crs = W.c_rs + (int64_t)c * d.RSW;
      wsync();
      for (int i = lane(); i < TW; i += kWave) o_opt[i] = inl ? lc.rem[(int64_t)c * TW + i] : gc.rem[(int64_t)c * TW + i];
      rec[RF_CLAIM] = c;  // wave-wide store of a uniform value
      {
        int cc = 0;
        for (int i = lane(); i < TW; i += kWave) cc += __popc(inl ? lc.rem[(int64_t)c * TW + i] : gc.rem[(int64_t)c * TW + i]);
        nopt = wred_add(cc);
      }
      const bool spot = rs_member(L, crs, d.ctKey, d.spotBit), od = rs_member(L, crs, d.ctKey, d.odBit);
      flags |= (spot ? RB_HAS_SPOT : 0) | (od ? RB_HAS_OD : 0);
      if (allSched && nclaims == 1) {
        if (W.cflags & CF_PRICE_ERR) {
          action = CA_ERROR;
        } else {
          // filterByPrice into LDS scratch (s_cand), then filterOutSameType into s_rem
          nprice = inl ? price_filter(lc.rem + (int64_t)c * TW, s_cand, tpl, crs, spot, od, W.price)
                       : price_filter(gc.rem + (int64_t)c * TW, s_cand, tpl, crs, spot, od, W.price);
          wsync();
          for (int i = lane(); i < TW; i += kWave) o_price[i] = s_cand[i];
          if (nprice > 0 && !((W.cflags & CF_ALL_SPOT) && spot)) {
            action = CA_REPLACE;
            const bool narrowed = spot && od;  // [spot, on-demand] -> spot (consolidation.go:183-188)
            if (narrowed) flags |= RB_NARROWED;
            if (W.cflags & CF_MULTI) {
              const int tb = s_tbeg[tpl], nIT = s_tbeg[tpl + 1] - tb;
              double mx = __DBL_MAX__;
              for (int pos = lane(); pos < nIT; pos += kWave)
                if ((s_cand[pos >> 5] >> (pos & 31)) & 1u) {
                  const double v = W.st_price[D.tpl_its[tb + pos]];
                  if (v == v && v < mx) mx = v;
                }
              for (int off = 32; off >= 1; off >>= 1) {
                const double x = __shfl_xor(mx, off);
                mx = x < mx ? x : mx;
              }
              nsame = price_filter(s_cand, s_rem, tpl, crs, spot, od && !narrowed, mx);
              wsync();
              for (int i = lane(); i < TW; i += kWave) o_same[i] = s_rem[i];
            }
          }
        }
      }
    } else if (allSched && nclaims == 0 && err == KE_OK) {
      action = CA_DELETE;
    }
    {  // wave-wide stores of uniform values
      rec[RF_FLAGS] = flags;
      rec[RF_NCLAIMS] = nclaims;
      rec[RF_HOSTINCR] = hostCtr;
      rec[RF_TPL] = tpl;
      rec[RF_HOST] = host;
      rec[RF_ACTION] = action;
      rec[RF_NOPT] = nopt;
      rec[RF_NPRICE] = nprice;
      rec[RF_NSAME] = nsame;
      rec[RF_ERROR] = err;
      rec[RF_ALGB_LO] = (int32_t)(uint32_t)(uint64_t)algbytes;
      rec[RF_ALGB_HI] = (int32_t)(uint32_t)((uint64_t)algbytes >> 32);
    }
  }

  // A simulation's queue state (what k_init does for a Solve), written at its first push-back: until then the
  // queue is the NewQueue order itself and every pod is pending in its first relaxation state, which the window
  // reads directly (refill's `ident`) -- most simulations never push a pod back and skip this.
  __device__ __forceinline__ void sim_queue_init(int P) {
    for (int i = lane(); i < P; i += kWave) {
      W.queue[i] = i;
      W.pod_state[i] = W.sstart ? W.sstart[W.pod_map[i]] : D.pod_state0[W.pod_map[i]];
      W.pod_status[i] = ST_PENDING;
      W.pod_fstate[i] = -1;
      W.last_len[i] = 0;
    }
    hbm_release();
    wsync();
  }

  // --- 64-pod queue window: one gather per 64 pops, one entry per lane ------------------------
  // ident: no pod was pushed back yet in this Solve, so every pod is in its first relaxation state, its
  // staleness word is 0, a simulation's pending status is untouched and its queue is still the identity:
  // the window reads the pods' first-state copies (pod_s0) instead of going through W.pod_state and the
  // state tables (one dependent memory level fewer per refill).
  __device__ __forceinline__ void refill(Window<RT>& w, int qhead, int qlen, int P, bool pushed, bool ident) {
    if (pushed) hbm_release();  // queue pushes / relaxation states / staleness words have landed
    const int n = qlen < kWave ? qlen : kWave;
    if (lane() < n) {
      int pos = qhead + lane();
      if (pos >= P) pos -= P;
      w.p = SIM && ident ? pos : ld_sc1(W.queue + pos);
      w.g = SIM ? W.pod_map[w.p] : w.p;
      w.uid = SIM ? w.p : D.pod_uid[w.p];  // simulations reject duplicate UIDs: local index == UID
      if (ident) {
        w.s = D.pod_state0[w.g];
        w.ll = 0;
        const uint64_t KS_G* s0 = D.pod_s0 + 4 * (int64_t)w.g;
        w.tol0 = s0[0];
        w.tol1 = s0[1];
        w.toltpl = s0[2];
        w.flags = (int)(uint32_t)s0[3];
        w.st = ST_PENDING;
      } else {
        w.s = ld_sc1(W.pod_state + w.p);
        w.ll = ld_sc1(W.last_len + w.uid);
        w.flags = D.st_flags[w.s];
        w.st = SIM ? ld_sc1(W.pod_status + w.p) : 0;
        w.toltpl = D.st_toltpl[w.s];
        w.tol0 = D.st_tol[2 * w.s];
        w.tol1 = D.st_tol[2 * w.s + 1];
      }
      w.pf = SIM || (!LEAN && d.volAny) ? D.pod_flags[w.g] : 0;
      w.rl = LEAN && ident ? W.run_len[pos] : 1;
      w.hpc = D.pod_hpc[w.g];
      w.hpu = D.pod_hpu[w.g];
      w.hpo = D.pod_hpo[w.g];
      if (TOPO) {
        w.tsel = D.pod_gsel[(int64_t)w.g * d.GMW];
        w.tinv = D.pod_ginv[(int64_t)w.g * d.GMW];
        w.town = D.st_gown[(int64_t)w.s * d.GMW];
        w.trss = rs_present(D.st_rss + (int64_t)w.s * d.RSW);
      }
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= d.R) break;
        w.req[r] = D.pod_req[(int64_t)w.g * R() + r];
      }
    }
  }
};

// --- Multi-wave simulations (MW) ------------------------------------------------------------------
// A long simulation (a multi-node prefix re-schedules thousands of pods as one dependent chain) runs on a
// 4-wave workgroup: wave 0 runs the simulation as the single-wave kernel does, and the register window's
// 64-node blocks are spread over the waves (wave k holds nodes [64k, 64k + 64)).  The window steps of the
// resource-only fast path are split by block: a run of identical pods computes each block's per-node
// capacity and scan on its own wave, the blocks' totals meet in an LDS mailbox, and each wave commits its
// block's shares; a single pod's first fit is one ballot per block.  Two workgroup barriers per step
// (parameters posted / block results posted).  Everything else -- queue, node scan past the window,
// NodeClaims, templates, relaxation, the decision -- stays on wave 0.  The helpers keep their
// AllNonPendingPodsScheduled and algorithmic-byte contributions and hand them over at MW_EXIT.
enum MwCmd : int { MW_RUN = 1, MW_FIT = 2, MW_EXIT = 3 };
enum MwSlot : int {  // uint32 words of the mailbox (LDS, after the plan's dynamic LDS)
  MB_CMD = 0, MB_SEQ = 1, MB_M = 2, MB_FPF = 3, MB_FT0 = 4, MB_FT1 = 6, MB_FP = 8,  // FP: 2 words per resource
  MB_TOT = 40, MB_MASK = 48, MB_UMASK = 56, MB_ALL = 64, MB_AB = 72, MB_WORDS = 80
};
constexpr int kMwWaves = 4;
constexpr size_t kMwBytes = 4 * MB_WORDS;
__device__ __forceinline__ void mb_st64(LU32 mb, int i, uint64_t v) {
  mb[i] = (uint32_t)v;
  mb[i + 1] = (uint32_t)(v >> 32);
}
__device__ __forceinline__ uint64_t mb_ld64(LU32 mb, int i) { return (uint64_t)mb[i] | ((uint64_t)mb[i + 1] << 32); }
__device__ __forceinline__ void mw_barrier() { __syncthreads(); }

// One 64-node block of the register window, free capacity form (FREEW): as k_solve's window init.
template <int RM>
struct MwBlock {
  uint64_t tx, ty;
  int64_t av[RM];
  int nf;
};
template <int RM>
__device__ __forceinline__ void mw_block_init(MwBlock<RM>& b, const KsDev& D, LU32 s_rmv, int kb) {
  const KsDims& d = D.d;
  const int n = kb * kWave + lane(), c = n < d.N ? n : d.N - 1;
  b.tx = D.n_taint[2 * c];
  b.ty = D.n_taint[2 * c + 1];
  bool never = n >= d.N || ((s_rmv[c >> 5] >> (c & 31)) & 1u) != 0;
#pragma unroll
  for (int r = 0; r < RM; r++) {
    const int64_t a = D.n_avail[(int64_t)c * RM + r], q = D.n_req0[(int64_t)c * RM + r];
    never |= a < 0;
    b.av[r] = a - q;
  }
#pragma unroll
  for (int r = 0; r < RM; r++) b.av[r] = never ? INT64_MIN : b.av[r];
  b.nf = D.n_flags[c];
}
// A run of m identical pods: this lane's node capacity for it (as the single-wave run step).
template <int RM>
__device__ __forceinline__ int mw_run_cap(const MwBlock<RM>& b, int m, const int64_t* fp, const float* rq, uint64_t ft0,
                                          uint64_t ft1) {
  const bool tol = (((b.tx & ~ft0) | (b.ty & ~ft1)) == 0);
  int cap = tol ? m : 0;
#pragma unroll
  for (int r = 0; r < RM; r++) {
    const int c = run_cap(b.av[r], fp[r], rq[r], m);
    cap = c < cap ? c : cap;
  }
  return cap;
}
// The lane's share of the run given the pods the blocks before this one take (base); branch-free.
template <int RM>
__device__ __forceinline__ int mw_run_commit(MwBlock<RM>& b, int base, int cap, int incl, int m, const int64_t* fp) {
  const int p0 = base + incl - cap, room = m - p0;
  const int tk = room <= 0 ? 0 : (cap < room ? cap : room);
#pragma unroll
  for (int r = 0; r < RM; r++) b.av[r] -= (int64_t)tk * fp[r];
  return tk;
}
template <int RM>
__device__ __forceinline__ bool mw_fits(const MwBlock<RM>& b, const int64_t* fp, uint64_t ft0, uint64_t ft1) {
  bool ok = (((b.tx & ~ft0) | (b.ty & ~ft1)) == 0);
#pragma unroll
  for (int r = 0; r < RM; r++) ok &= fp[r] <= b.av[r];
  return ok;
}
// The first block (in node order) whose ballot holds a fit: (block, its ballot), uniform; -1 if none.
__device__ __forceinline__ int mw_first_fit(LU32 mb, uint64_t& mj) {
  int kj = -1;
  mj = 0;
#pragma unroll
  for (int q = 0; q < kMwWaves; q++) {
    const uint64_t mq = mb_ld64(mb, MB_MASK + 2 * q);
    const bool take = kj < 0 && mq != 0;
    kj = take ? q : kj;
    mj = take ? mq : mj;
  }
  mj = (uint64_t)uni64((int64_t)mj);
  return uni(kj);
}

// Waves 1..3 of an MW simulation: their window block, the mailbox loop, then their contributions.
template <int RM>
__device__ __forceinline__ void mw_helper(const KsDev& D, const KsWork& W, LU32 s_rmv, LU32 mb, int k) {
  const int R = D.d.R;
  mw_barrier();  // B0a: wave 0's prologue (the removed-node mask) is in LDS
  MwBlock<RM> b;
  mw_block_init<RM>(b, D, s_rmv, k);
  mb_st64(mb, MB_UMASK + 2 * k, wballot(b.nf & NF_UNUSABLE));  // wave-wide store of a uniform value
  mw_barrier();  // B0b
  bool winUnusable = false;
#pragma unroll
  for (int q = 0; q < kMwWaves; q++) winUnusable |= mb_ld64(mb, MB_UMASK + 2 * q) != 0;
  winUnusable = ub(winUnusable);
  bool all = true;
  int64_t ab = 0;
  int seen = 0;
  // every wave-0 step posts a new sequence number; a bound on the steps and a stale number (wave 0 gone
  // without MW_EXIT, which the kernel never does) both end the loop, so no helper can outlive wave 0
  const int maxOps = 4 * W.P + 64;
  for (int it = 0; it < maxOps; it++) {
    mw_barrier();  // B1: a step's parameters are posted
    const int seq = uni((int)mb[MB_SEQ]), cmd = uni((int)mb[MB_CMD]);
    if (seq == seen) return;
    seen = seq;
    if (cmd == MW_EXIT) {
      mb[MB_ALL + k] = all ? 1u : 0u;  // wave-wide stores of uniform values
      mb_st64(mb, MB_AB + 2 * k, (uint64_t)ab);
      mw_barrier();  // B2
      return;
    }
    const int m = uni((int)mb[MB_M]), fpf = uni((int)mb[MB_FPF]);
    const uint64_t ft0 = (uint64_t)uni64((int64_t)mb_ld64(mb, MB_FT0)), ft1 = (uint64_t)uni64((int64_t)mb_ld64(mb, MB_FT1));
    int64_t fp[RM];
#pragma unroll
    for (int r = 0; r < RM; r++) fp[r] = uni64((int64_t)mb_ld64(mb, MB_FP + 2 * r));
    if (cmd == MW_RUN) {
      float rq[RM];
#pragma unroll
      for (int r = 0; r < RM; r++) rq[r] = run_rcp(fp[r]);
      const int cap = mw_run_cap<RM>(b, m, fp, rq, ft0, ft1);
      const int incl = wscan_add(cap);
      mb[MB_TOT + k] = (uint32_t)rdl(incl, kWave - 1);  // wave-wide store of a uniform value
      mw_barrier();  // B2: every block's total is posted
      int base = 0;
#pragma unroll
      for (int q = 0; q < kMwWaves; q++) base += q < k ? (int)mb[MB_TOT + q] : 0;
      base = uni(base);
      const int tk = mw_run_commit<RM>(b, base, cap, incl, m, fp);
      const bool unusable = tk > 0 && (b.nf & NF_UNUSABLE);
      if (winUnusable && !(fpf & PF_PROVISIONABLE) && wballot(unusable)) all = false;
      ab += (int64_t)rdl(wscan_add(tk * (k * kWave + lane() + 1)), kWave - 1) * (16 * R + 16);
    } else {  // MW_FIT: a single pod's first fit over the window
      mb_st64(mb, MB_MASK + 2 * k, wballot(mw_fits<RM>(b, fp, ft0, ft1)));
      mw_barrier();  // B2: every block's ballot is posted
      uint64_t mj;
      const int kj = mw_first_fit(mb, mj);
      if (kj == k) {
        const bool own = lane() == ctz64(mj);
#pragma unroll
        for (int r = 0; r < RM; r++) b.av[r] -= own ? fp[r] : 0;
      }
    }
  }
}

template <int RT, bool TL, bool SIM, bool TOPO, bool LEAN, bool MW = false, bool SLOG = false>
__global__ __attribute__((amdgpu_flat_work_group_size(1, MW ? 256 : 64))) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_solve(KsDev D, const KsWork* works, Plan pl) {
#define KS_BODY_WORK ((const KsWork KS_C*)works)[blockIdx.x]
#define KS_BODY_SMEM_DECL                                             \
  extern __shared__ __attribute__((aligned(16))) char smem_generic[]; \
  char KS_L* smem = (char KS_L*)smem_generic;
#include "ks_solve_body.inc"
#undef KS_BODY_WORK
#undef KS_BODY_SMEM_DECL
}

// The same body for one simulation of a mixed launch (k_sim_mixed): work item widx, LDS at smem_in.
template <int RT, bool TL, bool SIM, bool TOPO, bool LEAN, bool MW, bool SLOG = false>
__device__ __forceinline__ void solve_body(const KsDev& D, const KsWork* works, const Plan& pl, int widx,
                                           char KS_L* smem_in) {
#define KS_BODY_WORK ((const KsWork KS_C*)works)[widx]
#define KS_BODY_SMEM_DECL char KS_L* smem = smem_in;
#include "ks_solve_body.inc"
#undef KS_BODY_WORK
#undef KS_BODY_SMEM_DECL
}

// One launch for a consolidation pass with long simulations (MW): workgroups [0, nmw) run the long ones on
// 4 waves, dispatched first; each later workgroup runs four short ones, one per wave, each in its own LDS
// slice (stride bytes).  The two kinds overlap on the chip, which two launches on two streams did not.
template <int RT>
__global__ __attribute__((amdgpu_flat_work_group_size(1, 256))) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_sim_mixed(
    KsDev D, const KsWork* works, Plan pl, int nmw, int n, int stride) {
  extern __shared__ __attribute__((aligned(16))) char smem_mixed[];
  char KS_L* base = (char KS_L*)smem_mixed;
  if ((int)blockIdx.x < nmw) {
    solve_body<RT, true, true, false, true, true>(D, works, pl, (int)blockIdx.x, base);
  } else {
    const int wv = (int)(threadIdx.x >> 6);
    const int s = nmw + ((int)blockIdx.x - nmw) * kMwWaves + wv;
    if (s < n) solve_body<RT, true, true, false, true, false>(D, works, pl, s, base + (size_t)wv * stride);
  }
}

// Every translation unit instantiates one k_solve family (KS_TU 0: Solve, 1: Solve + topology,
// 2: simulations, 3: simulations + topology; ks_solve_topo.hip / ks_sim.hip / ks_sim_topo.hip
// include this file), so the four compile in parallel.  KS_TU 4 / 5 (ks_simlog.hip / ks_simlog_topo.hip) are the
// simulation families again with SLOG: the commit log is stored, for the re-run of one simulation whose placements
// the host renders (ks_cons.cpp rerun_logged).  Those are the single-wave routes only.
template <bool SIM, bool TOPO, bool SLOG = false>
hipError_t launch_family(const KsDev& D, const KsWork* works_dev, int n, const Plan& pl, hipStream_t st) {
#define KS_LAUNCH(RT_, TL_, LEAN_)                                                                                 \
  do {                                                                                                             \
    route_note(Route{SIM ? (SLOG ? (TOPO ? KR_SIMS_TOPO_LOG : KR_SIMS_LOG) : (TOPO ? KR_SIMS_TOPO : KR_SIMS))          \
                         : (TOPO ? KR_SOLVE_TOPO : KR_SOLVE),                                                      \
                     RT_, TL_, LEAN_, n, 0});                                                                      \
    hipLaunchKernelGGL((k_solve<RT_, TL_, SIM, TOPO, LEAN_, false, SLOG>), dim3(n), dim3(kWave), pl.lds, st, D,    \
                       works_dev, pl);                                                                             \
  } while (0)
  if (n <= 0) return hipSuccess;  // e.g. a consolidation pass with no candidates: nothing to simulate
  const bool tl = pl.talloc != 0;
  // the lean instantiations exist for the common shapes only: 3 or 4 resources, LDS-resident tables
  const bool lean = !TOPO && D.d.lean && tl;
  switch (D.d.R) {
    case 3: if (lean) KS_LAUNCH(3, true, !TOPO); else if (tl) KS_LAUNCH(3, true, false); else KS_LAUNCH(3, false, false); break;
    case 4: if (lean) KS_LAUNCH(4, true, !TOPO); else if (tl) KS_LAUNCH(4, true, false); else KS_LAUNCH(4, false, false); break;
    default: if (tl) KS_LAUNCH(0, true, false); else KS_LAUNCH(0, false, false); break;
  }
#undef KS_LAUNCH
  return hipGetLastError();
}
using FamilyFn = hipError_t (*)(const KsDev&, const KsWork*, int, const Plan&, hipStream_t);
hipError_t launch_solve_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_solve_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_sims_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_sims_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_sims_mw(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_sims_mixed(const KsDev& D, const KsWork* w, int n, int nmw, const Plan& pl, hipStream_t st);
hipError_t launch_simlog_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);
hipError_t launch_simlog_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st);

#if KS_TU == 1
hipError_t launch_solve_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<false, true>(D, w, n, pl, st);
}
#elif KS_TU == 2
hipError_t launch_sims_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<true, false>(D, w, n, pl, st);
}
// One mixed launch (k_sim_mixed): the first nmw simulations on 4-wave workgroups, the rest four to a workgroup.
// hipErrorNotSupported when four LDS slices do not fit a CU (the caller falls back to two launches).
hipError_t launch_sims_mixed(const KsDev& D, const KsWork* w, int n, int nmw, const Plan& pl, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const size_t stride = (pl.lds + 15) & ~(size_t)15;
  const size_t lds = std::max(pl.lds + kMwBytes, (size_t)kMwWaves * stride);
  if (D.d.G || !D.d.lean || !pl.talloc || D.d.N <= 0 || lds > 160 * 1024) return hipErrorNotSupported;
  const int grid = nmw + (n - nmw + kMwWaves - 1) / kMwWaves;
  const dim3 blk(kMwWaves * kWave);
  if (D.d.R == 3 || D.d.R == 4) route_note(Route{KR_SIMS_MIXED, D.d.R, 1, 1, n, nmw});
  switch (D.d.R) {
    case 3: hipLaunchKernelGGL((k_sim_mixed<3>), dim3(grid), blk, lds, st, D, w, pl, nmw, n, (int)stride); break;
    case 4: hipLaunchKernelGGL((k_sim_mixed<4>), dim3(grid), blk, lds, st, D, w, pl, nmw, n, (int)stride); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}
// The long simulations on 4-wave workgroups (MW): resource-only pods with the window in free-capacity form
// (the LEAN instantiations); hipErrorNotSupported for other problems (the caller runs them single-wave).
hipError_t launch_sims_mw(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (D.d.G || !D.d.lean || !pl.talloc || D.d.N <= 0 || pl.lds + kMwBytes > 160 * 1024) return hipErrorNotSupported;
  const dim3 blk(kMwWaves * kWave);
  if (D.d.R == 3 || D.d.R == 4) route_note(Route{KR_SIMS_MW, D.d.R, 1, 1, n, 0});
  switch (D.d.R) {
    case 3: hipLaunchKernelGGL((k_solve<3, true, true, false, true, true>), dim3(n), blk, pl.lds + kMwBytes, st, D, w, pl); break;
    case 4: hipLaunchKernelGGL((k_solve<4, true, true, false, true, true>), dim3(n), blk, pl.lds + kMwBytes, st, D, w, pl); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}
#elif KS_TU == 3
hipError_t launch_sims_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<true, true>(D, w, n, pl, st);
}
#elif KS_TU == 4
hipError_t launch_simlog_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<true, false, true>(D, w, n, pl, st);
}
#elif KS_TU == 5
hipError_t launch_simlog_topo(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<true, true, true>(D, w, n, pl, st);
}
#else
hipError_t launch_solve_plain(const KsDev& D, const KsWork* w, int n, const Plan& pl, hipStream_t st) {
  return launch_family<false, false>(D, w, n, pl, st);
}

// LDS plan.  Position-indexed state (order, pod count, template, headroom) bounds the NodeClaims
// per Solve (KO); claims [0, KL) also keep their template/requests/max/options/thresholds in LDS,
// the rest in HBM.  The instance-type tables go to LDS first when they leave room for 64 claims.
// One-Solve launches use the whole 160 KiB of a CU; batched simulations pass a smaller budget.
// wideKO: a Solve that created more NodeClaims than the default plan holds is re-planned with 64 LDS-resident
// claims and the rest of the LDS given to claim positions: level 1 keeps the instance-type tables in LDS, level 2
// (when 1 still holds too few) moves them to HBM.  C3 (844 NodeClaims): 56.0k -> 59.1k pods/s at level 1.
static Plan make_plan_live(const KsDims& d, size_t budget, bool sim, int wideKO, bool live, int frontTotal);
Plan make_plan(const KsDims& d, size_t budget, bool sim, int wideKO, int frontTotal) {
  // The live node list serves the non-LEAN Solve instantiations with a register window (RT 3 or 4, launch_family):
  // a lean problem runs LEAN whenever its instance-type tables fit in LDS (talloc), so its plan reserves the list
  // only when they do not.
  const bool rt = d.R == 3 || d.R == 4;
  if (sim || !rt) return make_plan_live(d, budget, sim, wideKO, false, frontTotal);
  if (d.lean) {
    const Plan lean = make_plan_live(d, budget, sim, wideKO, false, frontTotal);
    if (lean.talloc) return lean;
  }
  return make_plan_live(d, budget, sim, wideKO, true, frontTotal);
}

static Plan make_plan_live(const KsDims& d, size_t budget, bool sim, int wideKO, bool live, int frontTotal) {
  auto r16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  Plan pl{};
  const size_t R = d.R, TW = d.TW, tot = d.totalTplIts;
  const size_t fixed = r16(sizeof(KeyMeta) * d.NK) + r16(4 * (size_t)(d.NTPL + 1)) + r16(8 * (size_t)(d.NPOOL + 1) * R) +
                       2 * r16(4 * (size_t)d.RSW) + 5 * r16(4 * TW + 8) + 16 * 16 + (d.volAny ? 48 : 0) +
                       (KS_TPL_MEMO && !sim && d.lean ? r16(4 * (size_t)tpl_memo_words((int)R, (int)TW)) : 0) +
                       (KS_RUN_FRONT && KS_CLAIM_RUNS && !sim && d.lean ? r16(4 * (size_t)(d.NTPL + 1)) + r16(4 * (size_t)frontTotal) : 0) +
                       (sim ? 4 * r16(4 * (size_t)((d.N + 31) / 32)) : d.fnOn ? r16(4 * (size_t)((d.N + 31) / 32)) : 0) +
                       (d.G ? r16(4 * (size_t)d.G * TGM_WORDS) + r16(4 * (size_t)d.G) + 2 * r16(4 * (size_t)d.RSW) +
                                  (d.GMW > 1 ? r16(8 * (size_t)GS_N * d.GMW) : 0) +
                                  (sim ? r16(4 * (size_t)((d.tgCntWords - d.tgSmall + 31) / 32)) + 4 * kTdwKeys * kTdw : 0)
                              : 0);
  const size_t posB = 16 + 8 * R;                        // order, okey, ptpl, phead (+ rounding)
  const size_t clmB = 16 + 16 * R + 4 * TW + 4 * R;      // tpl, cnt, req, max, rem, thr (+ rounding)
  const size_t slack = 10 * 16;                          // per-array 16-byte rounding
  const size_t tallocB = r16(8 * tot * R);
  const size_t tsortB = r16(8 * tot * R) + r16(4 * tot * R);
  size_t avail = budget > fixed + slack ? budget - fixed - slack : 0;
  // The topology count table's LDS-resident prefix: the small-key groups; a Solve also keeps the
  // hostname groups there when the whole table takes at most a quarter of what is left (a simulation's
  // hostname counts are copy-on-write over the shared HBM table instead).
  pl.tcl = d.G ? d.tgSmall : 0;
  if (d.G && !sim && 4 * (size_t)d.tgCntWords <= avail / 4) pl.tcl = d.tgCntWords;
  const size_t tclB = r16(4 * (size_t)pl.tcl);
  avail = avail > tclB ? avail - tclB : 0;
  // the node domain table likewise (a Solve's first-fit scan reads it for every node and matching group)
  const size_t tdWords = (size_t)d.TK * (size_t)d.N;
  pl.tdl = d.G && !sim && tdWords > 0 && 4 * tdWords <= avail / 4 ? (int32_t)tdWords : 0;
  const size_t tdlB = r16(4 * (size_t)pl.tdl);
  avail = avail > tdlB ? avail - tdlB : 0;
  // a Solve's live node list: the existing nodes past the register window passing Fits for the current
  // request vector (ks_solve_body.inc)
  pl.livl = live && d.N > 0 && !d.negReq && !d.tgUnlab && 4 * (size_t)d.N <= avail / 4 ? d.N : 0;
  const size_t livB = r16(4 * (size_t)pl.livl);
  avail = avail > livB ? avail - livB : 0;
  // The threshold filter needs the sorted lists only without negative requests.
  const size_t tablesB = tallocB + (d.negReq ? 0 : tsortB);
  pl.talloc = (wideKO < 2 && tablesB + 64 * (posB + clmB) <= avail) ? 1 : 0;
  pl.tsort = pl.talloc && !d.negReq;
  if (pl.talloc) avail -= tablesB;
  // The LEAN Solve's per-template requirement / offering bitsets (KS_TPL_MASKS), when they too leave room for 64
  // claims; without them a NewNodeClaim that misses the memo derives both again.
  const size_t tmaskB = tpl_mask_bytes(d.NTPL, (int)TW);
  pl.tmask = (KS_TPL_MASKS && !sim && d.lean && pl.talloc && tpl_mask_fits(avail, d.NTPL, (int)TW, posB, clmB)) ? 1 : 0;
  if (pl.tmask) avail -= tmaskB;
  const size_t kAll = avail / (posB + clmB);
  size_t ko, kl;
  if (kAll >= (size_t)d.Kcap) {
    ko = kl = d.Kcap;
  } else if (wideKO) {  // 64 LDS-resident claims, the rest to positions (C3: 8-96 claims measured within 1.5 %)
    kl = std::min<size_t>(64, kAll);
    ko = std::min((size_t)d.Kcap, (avail - kl * clmB) / posB);
  } else {  // half the LDS to positions, half to claim state
    ko = std::min((size_t)d.Kcap, std::max(kAll, avail / 2 / posB));
    kl = std::min(ko, (avail - ko * posB) / clmB);
  }
  pl.KO = (int)ko;
  pl.KL = (int)kl;
  pl.lds = fixed + tclB + tdlB + livB + 3 * r16(4 * ko) + r16(8 * ko * R) + 2 * r16(4 * kl) + 2 * r16(8 * kl * R) + r16(4 * kl * TW) +
           r16(4 * kl * R) + (pl.tsort ? tsortB : 0) + (pl.talloc ? tallocB : 0) + (pl.tmask ? tmaskB : 0);
  return pl;
}

int run_fuse_build() { return KS_RUN_FUSE; }
int tpl_masks_build() { return KS_TPL_MASKS; }
int log_runs_build() { return KS_LOG_RUNS && KS_CLAIM_RUNS; }
int sort_leaf_build() { return KS_SORT_LEAF && !KS_SORT_LANE0; }
int closed_shift_build() { return KS_CLOSED_SHIFT && KS_SORT_CLOSED; }
int pivot_arith_build() { return KS_PIVOT_ARITH && KS_SORT_CLOSED; }
int pivot_arith_check_build() { return KS_PIVOT_ARITH_CHECK && KS_SORT_CLOSED; }
int append_closed_build() { return KS_APPEND_CLOSED && KS_SORT_CLOSED; }
int cross_quick_from_build() { return KS_CROSS_QUICK_FROM && KS_SORT_CLOSED && KS_RUN_CROSS && KS_CLAIM_RUNS && !KS_RUN_FUSE; }
int sort_regs_build() { return KS_SORT_REGS != 0 && KS_SORT_OUTLINE; }
int sort_regs_n64_build() { return sort_regs_build() && KS_SORT_REGS_N64; }
int cap_bound_build() { return KS_CAP_BOUND && KS_CLAIM_RUNS; }
int thr_batch_build() { return KS_THR_BATCH; }
int run_chain_build() { return KS_RUN_CHAIN && KS_CLAIM_RUNS; }

// Test / diagnostic kernel (ks_claim_sort_probe): Solver::sort_claims' logic on arrays of the caller's choosing,
// one wave, no Solve.  keys / order [n] are loaded into LDS with the position arrays ptpl / phead gathered from the
// claim tables ctpl [n] / chead [n][R] (by claim id); mode 0 sorts as for an appended claim (pos -1), mode 1 as
// after a count increment at pos, taking the closed form where sort_claims does, mode 2 as for an appended claim
// that sort_claims is told of (`app`: KS_APPEND_CLOSED); all four arrays are written back with how it was done
// (Solver::SORT_*).
template <int R>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_claim_sort_probe(
    int32_t* keys, int32_t* order, int n, int mode, int pos, const int32_t* ctpl, const int64_t* chead, int32_t* ptpl,
    int64_t* phead, int32_t* how) {
  extern __shared__ __attribute__((aligned(16))) char smem_probe[];
  char KS_L* sp = (char KS_L*)smem_probe;
  const size_t n4 = (4 * (size_t)n + 15) & ~(size_t)15;
  ClaimSort cs;
  LI64 s_phead = (LI64)sp;
  cs.s_okey = (LI32)(sp + 8 * (size_t)n * R);
  cs.s_order = (LI32)(sp + 8 * (size_t)n * R + n4);
  LI32 s_ptpl = (LI32)(sp + 8 * (size_t)n * R + 2 * n4);
  auto gather = [&](int lo, int hi) {  // sort_claims' regather over positions [lo, hi]
    for (int j = lo + lane(); j <= hi; j += kWave) {
      const int c = cs.s_order[j];
      s_ptpl[j] = ctpl[c];
      for (int r = 0; r < R; r++) s_phead[(int64_t)j * R + r] = chead[(int64_t)c * R + r];
    }
    wsync();
  };
  for (int j = lane(); j < n; j += kWave) {
    cs.s_okey[j] = keys[j];
    cs.s_order[j] = order[j];
  }
  wsync();
  gather(0, n - 1);
  if (mode != 1) pos = -1;
  int tlo = n, thi = -1, pivot = -1, res = 1;
  bool closed = false, appc = false;
  if (KS_APPEND_CLOSED && KS_SORT_CLOSED && mode == 2 && n >= 50) {  // sort_claims' `app`
    appc = cs.append_closed<R>(n, s_ptpl, s_phead) >= 0;  // (all four arrays moved: nothing to regather)
    if (appc) res = 0;
  }
  if (n > 12 && !appc) {
    int hint = 0, pv = 0, ts = -1;
    bool arith = false;
    constexpr bool PA = KS_PIVOT_ARITH && KS_SORT_CLOSED;
    if (KS_CLOSED_SHIFT && KS_SORT_CLOSED) ts = cs.closed_crossing<R, PA>(n, pos, s_ptpl, s_phead, hint, pv, arith);
    else {
      if (PA && pos >= 0 && n >= 50 && pos + 1 < n && !ClaimSort::pivot_sampled(n, pos)) {
        const int t = cs.closed_move(n, pos);
        if (t >= 0) {
          arith = closed = true;
          tlo = pos;
          thi = pos + t;
        }
      }
      if (!arith) pv = cs.w_choose_pivot(0, n, hint);
    }
    if (hint == 1) {
      pivot = pv;
      if (ts >= 0) closed = true;  // (nothing to regather)
      else if (KS_SORT_CLOSED && !KS_CLOSED_SHIFT && !PA && pos >= 0 && n >= 50 && pos + 1 < n) {
        const int t = cs.closed_move(n, pos);
        if (t >= 0) {
          closed = true;
          tlo = pos;
          thi = pos + t;
        }
      }
    }
  }
  int path = 0;  // the general re-sort's (KS_SORT_REGS): 1 finished on the register copy, 2 abandoned on a failed
                 // invariant, 3 more entries than the copy holds (2 and 3: the LDS code sorted)
  if (closed) res = 2;
  else if (!appc) {
    const uint32_t g = claim_sort_general<true, true>(cs.s_okey, cs.s_order, n, pivot);
    tlo = (int)(g & 0x7fff);
    thi = (int)(g >> 15 & 0x7fff) - 1;
    res = g >> 30 & 1 ? 0 : 1;
    path = g & kSortRegsDone ? 1 : KS_SORT_REGS == 0 ? 0 : n > (KS_SORT_REGS_N64 ? 64 : kSortRegsMax) ? 3 : 2;
  }
  wsync();
  gather(tlo, thi);
  for (int j = lane(); j < n; j += kWave) {
    keys[j] = cs.s_okey[j];
    order[j] = cs.s_order[j];
    ptpl[j] = s_ptpl[j];
    for (int r = 0; r < R; r++) phead[(int64_t)j * R + r] = s_phead[(int64_t)j * R + r];
  }
  how[lane()] = lane() == 1 ? path : lane() == 2 ? (int)appc : res;  // [kWave]: how, in word 1 the path, in word 2
                                                                     // whether the appended claim's closed form ran
}
// n <= kProbeMaxN positions, R 3 or 4 (the LEAN Solve's resource counts); the arrays are device pointers
hipError_t claim_sort_probe(int32_t* keys, int32_t* order, int n, int mode, int pos, int R, const int32_t* ctpl,
                            const int64_t* chead, int32_t* ptpl, int64_t* phead, int32_t* how, hipStream_t st) {
  if (n < 0 || n > kProbeMaxN || (R != 3 && R != 4)) return hipErrorInvalidValue;
  const size_t lds = 8 * (size_t)n * R + 3 * ((4 * (size_t)n + 15) & ~(size_t)15) + 16;
  if (R == 3) hipLaunchKernelGGL((k_claim_sort_probe<3>), dim3(1), dim3(kWave), lds, st, keys, order, n, mode, pos, ctpl, chead, ptpl, phead, how);
  else hipLaunchKernelGGL((k_claim_sort_probe<4>), dim3(1), dim3(kWave), lds, st, keys, order, n, mode, pos, ctpl, chead, ptpl, phead, how);
  return hipGetLastError();
}

// The LEAN Solve's fresh-NodeClaim table (KS_TPL_TABLE): one wave per (request class, template) runs the derivation
// try_templates would run on the Solve's one-wave chain (Solver::fresh_record) and writes its memo record to
// table[(class * NTPL + t) * tpl_memo_words]; blk is the block's base (ks_problem.h tpl_block_*), the class count the
// grid's.  Templates with a NodePool limit are never looked up (the memo's conditions); their records stay as the
// upload zeroed them.  The instance-type tables are read from HBM (TL false):
// a wave needs the key metadata, the template offsets and fronts and the scratch bitsets in LDS, nothing else.
template <int RT>
__global__ __attribute__((amdgpu_flat_work_group_size(64, 64))) void k_fresh_claims(KsDev D, const KsWork* works, Plan pl,
                                                                                    uint32_t* blk) {
  extern __shared__ __attribute__((aligned(16))) char smem_fresh[];
  const KsDims& d = D.d;
  const int cls = (int)blockIdx.x / d.NTPL, t = (int)blockIdx.x % d.NTPL;
  if (D.tpl_pool[t] >= 0) return;
  Solver<RT, false, false, false, true> S(D, ((const KsWork KS_C*)works)[0], pl);
  char KS_L* sp = (char KS_L*)smem_fresh;
  auto take = [&](size_t bytes) { char KS_L* r = sp; sp += (bytes + 15) & ~(size_t)15; return r; };
  KeyMeta KS_L* s_keys = (KeyMeta KS_L*)take(sizeof(KeyMeta) * d.NK);
  S.s_tbeg = (LI32)take(4 * (size_t)(d.NTPL + 1));
  S.s_fbeg = (LI32)take(4 * (size_t)(d.NTPL + 1));
  S.s_front = (LI32)take(4 * (size_t)D.frontTotal);
  S.s_rs = (LU32)take(4 * (size_t)d.RSW);
  S.s_rem = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_fic = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_fof = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_firr = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_memo = (LU32)take(4 * (size_t)tpl_memo_words(RT, d.TW));
  for (int i = lane(); i < d.NK * (int)(sizeof(KeyMeta) / 4); i += kWave)
    ((uint32_t KS_L*)s_keys)[i] = ((const uint32_t KS_G*)D.keys)[i];
  for (int i = lane(); i <= d.NTPL; i += kWave) {
    S.s_tbeg[i] = D.tpl_it_beg[i];
    S.s_fbeg[i] = D.tpl_front_beg[i];
  }
  for (int i = lane(); i < D.frontTotal; i += kWave) S.s_front[i] = D.tpl_front[i];
  S.L.nkeys = d.NK;
  S.L.W = d.W;
  S.L.NB = d.NB;
  S.L.HDR = d.HDR;
  S.L.RSW = d.RSW;
  S.L.keys = s_keys;
  S.L.wordValid = D.wordValid;
  S.L.vIsInt = D.vIsInt;
  S.L.vInt = D.vInt;
  wsync();
  const int nw = tpl_memo_words(RT, d.TW), ncls = (int)gridDim.x / d.NTPL;
  const int64_t KS_G* class_req = (const int64_t KS_G*)((const uint32_t KS_G*)blk + tpl_block_req(d.P, ncls, d.NTPL, nw));
  int64_t pod[RT];
#pragma unroll
  for (int r = 0; r < RT; r++) pod[r] = class_req[(int64_t)cls * RT + r];
  S.fresh_record(t, pod);
  uint32_t KS_G* out = (uint32_t KS_G*)blk + tpl_block_table(d.P) + (int64_t)blockIdx.x * nw;
  for (int i = lane(); i < nw; i += kWave) out[i] = S.s_memo[i];
}
int tpl_table_build() { return KS_TPL_TABLE && !KS_TPL_MASKS && KS_TPL_MEMO; }
int tpl_table_check_build() { return tpl_table_build() && KS_TPL_TABLE_CHECK; }
// ncls x NTPL waves; blk: the block's base on the device (pod_class and class_req uploaded, the table zeroed).  R 3 or
// 4: the LEAN Solve's resource counts (launch_family).
hipError_t launch_fresh_claims(const KsDev& D, const KsWork* works, const Plan& pl, uint32_t* blk, int ncls, hipStream_t st) {
  const KsDims& d = D.d;
  if (ncls <= 0 || d.NTPL <= 0 || (d.R != 3 && d.R != 4)) return hipErrorInvalidValue;
  auto r16 = [](size_t b) { return (b + 15) & ~(size_t)15; };
  const size_t lds = r16(sizeof(KeyMeta) * d.NK) + 2 * r16(4 * (size_t)(d.NTPL + 1)) + r16(4 * (size_t)D.frontTotal) +
                     r16(4 * (size_t)d.RSW) + 4 * r16(4 * (size_t)d.TW + 8) + r16(4 * (size_t)tpl_memo_words(d.R, d.TW));
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(ncls * d.NTPL));
  if (d.R == 3) hipLaunchKernelGGL((k_fresh_claims<3>), grid, dim3(kWave), lds, st, D, works, pl, blk);
  else hipLaunchKernelGGL((k_fresh_claims<4>), grid, dim3(kWave), lds, st, D, works, pl, blk);
  return hipGetLastError();
}

void launch_feasibility(const KsDev& D, hipStream_t st) {
  const int rows = D.d.S * D.d.NTPL;
  if (D.d.TW <= 32) {  // two rows per wave step
    const int blocks = std::min(2048, (rows + 7) / 8);
    hipLaunchKernelGGL(k_feasibility<32>, dim3(blocks), dim3(256), 0, st, D);
  } else {
    const int blocks = std::min(2048, (rows + 3) / 4);
    hipLaunchKernelGGL(k_feasibility<64>, dim3(blocks), dim3(256), 0, st, D);
  }
}

void launch_feasibility_nodes(const KsDev& D, hipStream_t st) {
  const int nbx = (D.d.N + 255) / 256;
  hipLaunchKernelGGL(k_feasibility_nodes, dim3(D.d.FNR * nbx), dim3(256), 0, st, D, nbx);
}

hipError_t queue_sort(const KsDev& D, uint64_t* keys, int32_t* vals, void* temp, size_t tempBytes, int32_t* out,
                      hipStream_t st);
hipError_t sim_run_lengths(const int32_t* podmap, const int32_t* entry_sim, const int64_t* pod_req, const uint64_t* pod_s0,
                           const int32_t* pod_flags, int R, int n, uint64_t* words, int32_t* run_len, hipStream_t st,
                           bool strict);

// One ks_solve: queue sort -> workspace init -> [mid event] -> k_solve (all on one stream).
// Topology problems get their own instantiation: the group state would otherwise occupy SGPRs (and
// their spills) across the whole commit loop of every topology-free Solve.
// fixed_order: NewQueue's order computed on the host (pods tying on the whole sort key), no radix sort.
// run_len / run_words (LEAN problems): the identical pods left in each queue position's run, which the LEAN
// Solve's claim runs read while nothing has been pushed back (they may then reach past the queue window).
hipError_t launch_solve(const KsDev& D, const KsWork* works_dev, int nrep, const Plan& pl, int32_t* qorder,
                        uint64_t* skeys, int32_t* svals, void* stemp, size_t stempBytes, hipStream_t st,
                        hipEvent_t mid, const int32_t* fixed_order, hipEvent_t* feas, int32_t* run_len,
                        uint64_t* run_words, hipEvent_t post) {
  if (pl.lds > 160 * 1024) return hipErrorInvalidValue;
  if (!fixed_order) {
    hipError_t e = queue_sort(D, skeys, svals, stemp, stempBytes, qorder, st);
    if (e != hipSuccess) return e;
  }
  if (D.d.lean && run_len && run_words) {
    hipError_t e = sim_run_lengths(fixed_order ? fixed_order : qorder, nullptr, D.pod_req, D.pod_s0, D.pod_flags, D.d.R,
                                   D.d.P, run_words, run_len, st, true);
    if (e != hipSuccess) return e;
  }
  if (D.d.fmOn) {
    if (feas) (void)hipEventRecord(feas[0], st);
    launch_feasibility(D, st);
    if (feas) (void)hipEventRecord(feas[1], st);
  }
  if (D.d.fnOn) {
    if (feas) (void)hipEventRecord(feas[2], st);
    launch_feasibility_nodes(D, st);
    if (feas) (void)hipEventRecord(feas[3], st);
  }
  hipLaunchKernelGGL(k_init, dim3(512), dim3(256), 0, st, D, works_dev, nrep,
                     fixed_order ? fixed_order : (const int32_t*)qorder);
  if (mid) (void)hipEventRecord(mid, st);
  hipError_t e = (D.d.G ? launch_solve_topo : launch_solve_plain)(D, works_dev, nrep, pl, st);
  if (post) (void)hipEventRecord(post, st);  // k_solve ends here
  // KS_LOG_RUNS: a LEAN Solve (launch_family's choice) logged its long runs as records; their entries are written now.
  // The grid is fixed by P -- the record count stays on the device.
  const bool leanRoute = !D.d.G && D.d.lean && pl.talloc && (D.d.R == 3 || D.d.R == 4);
  if (e == hipSuccess && log_runs_build() && leanRoute && nrep > 0 && D.d.P > 0) {
    const int bx = std::min(256, std::max(1, (D.d.P + 255) / 256)), by = std::min(nrep, 1024);
    hipLaunchKernelGGL(k_log_expand, dim3(bx, by), dim3(256), 0, st, works_dev, nrep,
                       fixed_order ? fixed_order : (const int32_t*)qorder, D.d.P);
    e = hipGetLastError();
  }
  return e;
}

// A batch of consolidation simulations (one wavefront each); their pod_map lists must already be
// in NewQueue order (sim_queue_sort).
hipError_t launch_sims(const KsDev& D, const KsWork* works_dev, int nsims, const Plan& pl, hipStream_t st) {
  if (pl.lds > 160 * 1024) return hipErrorInvalidValue;
  if (nsims <= 0) return hipSuccess;
  if (D.d.fmOn) launch_feasibility(D, st);
  if (D.d.fnOn) launch_feasibility_nodes(D, st);
  return (D.d.G ? launch_sims_topo : launch_sims_plain)(D, works_dev, nsims, pl, st);
}
// launch_sims on the logging instantiations (SLOG: the commit log is stored; KsWork::c_npods must be set).
hipError_t launch_sims_logged(const KsDev& D, const KsWork* works_dev, int nsims, const Plan& pl, hipStream_t st) {
  if (pl.lds > 160 * 1024) return hipErrorInvalidValue;
  if (nsims <= 0) return hipSuccess;
  if (D.d.fmOn) launch_feasibility(D, st);
  if (D.d.fnOn) launch_feasibility_nodes(D, st);
  return (D.d.G ? launch_simlog_topo : launch_simlog_plain)(D, works_dev, nsims, pl, st);
}
bool sims_mw_supported(const KsDev& D, const Plan& pl) {
  return !D.d.G && D.d.lean && pl.talloc && D.d.N > 0 && pl.lds + kMwBytes <= 160 * 1024 && (D.d.R == 3 || D.d.R == 4);
}
// The first nmw simulations (the long ones) on 4-wave workgroups on st2, the rest single-wave on st,
// concurrently: st2 waits for st's work so far (fork), st waits for st2 at the end (join).
hipError_t launch_sims_split(const KsDev& D, const KsWork* works_dev, int nsims, int nmw, const Plan& pl, hipStream_t st,
                             hipStream_t st2, hipEvent_t fork, hipEvent_t join) {
  if (nmw <= 0 || !sims_mw_supported(D, pl)) return launch_sims(D, works_dev, nsims, pl, st);
  if (pl.lds > 160 * 1024) return hipErrorInvalidValue;
  if (D.d.fmOn) launch_feasibility(D, st);
  if (D.d.fnOn) launch_feasibility_nodes(D, st);
  // one launch when four simulations' LDS fit a workgroup: the long ones are dispatched first
  const hipError_t em = launch_sims_mixed(D, works_dev, nsims, nmw, pl, st);
  if (em != hipErrorNotSupported) return em;
  hipError_t e = hipEventRecord(fork, st);
  if (e == hipSuccess) e = hipStreamWaitEvent(st2, fork, 0);
  if (e == hipSuccess) e = launch_sims_mw(D, works_dev, nmw, pl, st2);
  if (e == hipSuccess && nsims > nmw) e = launch_sims_plain(D, works_dev + nmw, nsims - nmw, pl, st);
  if (e == hipSuccess) e = hipEventRecord(join, st2);
  if (e == hipSuccess) e = hipStreamWaitEvent(st, join, 0);
  return e;
}
#endif

}  // namespace ks
