// ks_disrupt.h — the output layout of k_disrupt_pick (ks_disrupt.hip), shared with its host reader (ks_cons.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include "ks_problem.h"

namespace ks {

// out (int32 words): [DH_WORDS] header, [npos] one word per position, then disrupt_claim_words() words per NodeClaim of the
// picked simulation in s.newNodeClaims order: template, hostname ordinal, option count, [TW] options,
// [2R] requests (int64, low word first), [RSW] requirements.
//   slot[i]    launch slot (record / workspace index) of position i of the method's order
//   header     DH_PICK    first position with RF_ERROR == KE_OK and RB_ALL_SCHEDULED, -1: none
//              DH_ERRPOS  first position whose record reports a kernel error, -1: none; DH_ERR its code
//              DH_NCLAIMS / DH_NLOG of the picked simulation (its workspace counters)
//              DH_NEED    the words the whole output takes; claims are exported only when it is <= cap
//              DH_BAD     claim ids of `order` outside the workspace (never, unless a device store was lost)
//   position   (RF_NCLAIMS << 8) | (RF_FLAGS & 0xff)
// One 256-lane workgroup.  Stores of wave-uniform values are wave-wide, per-lane state is updated by select, and
// every store index is tested against `cap` (and a claim id against the workspace's capacity) before use.
enum DisruptHdr { DH_PICK = 0, DH_ERRPOS, DH_ERR, DH_NCLAIMS, DH_NLOG, DH_NEED, DH_BAD, DH_EXPORTED, DH_WORDS = 8 };
constexpr int kNoPos = 0x7fffffff;
KS_HD int disrupt_claim_words(int R, int TW, int RSW) { return 3 + TW + 2 * R + RSW; }

hipError_t disrupt_pick(const int32_t* recs, int recWords, const KsWork* works, const int32_t* slot, int npos, int R,
                        int TW, int RSW, int32_t* out, int cap, hipStream_t st);

}  // namespace ks
