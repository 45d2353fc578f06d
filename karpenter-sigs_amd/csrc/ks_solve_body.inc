// The body of k_solve (ks_solve.hip): one simulation or Solve per wavefront (MW: per 4-wave workgroup).
// Included by the k_solve kernel and by solve_body (the mixed simulation launch), which define
// KS_BODY_WORK (this workgroup's / wave's KsWork) and KS_BODY_SMEM_DECL (its LDS base `smem`).
  constexpr int RM = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::RM;
  // The loop's branch conditions are forced scalar (ub / uni): its control flow is wave-uniform by
  // construction, and left to prove that itself the compiler falls back to exec-masked code for the whole
  // commit loop, which costs time and, in one build of the requirement-carrying instantiation, lost a
  // claim-state write-back (two reference Binpacking scenarios; device requests 0 for one NodeClaim).
  // The LEAN Solve instantiation (resource-only pods, C1/C2) keeps the compiler's choice: there the
  // scalar form's extra SGPR spills cost 15 % of C2, and its parity is pinned by the full-size digests.
  // Round 6: with this compiler the Solves and the topology simulations are faster with the compiler's choice (C3
  // 58.9k -> 64.4k pods/s, C4 151k -> 159k, C5 + topology 10.8 -> 10.1 ms) and the whole GPU suite -- the reference
  // Binpacking scenarios among it -- is green on that build; the LEAN simulations (C5) stay forced (0.119 against
  // 0.125 ms).  -DKS_FORCE_UNIFORM restores round 5's choice.
#ifdef KS_FORCE_UNIFORM
  constexpr bool FORCEU = SIM || !LEAN;
#else
  constexpr bool FORCEU = SIM && LEAN;
#endif
  auto U = [](bool x) { return FORCEU ? ub(x) : x; };
  auto UI = [](int x) { return FORCEU ? uni(x) : x; };
  KS_BODY_SMEM_DECL
  const KsWork KS_C& W = KS_BODY_WORK;
  const KsDims& d = D.d;
  Solver<RT, TL, SIM, TOPO, LEAN, SLOG> S(D, W, pl);
  const int R = S.R();
  char KS_L* sp = smem;
  auto take = [&](size_t bytes) { char KS_L* r = sp; sp += (bytes + 15) & ~(size_t)15; return r; };
  KeyMeta KS_L* s_keys = (KeyMeta KS_L*)take(sizeof(KeyMeta) * d.NK);
  S.s_order = (LI32)take(4 * (size_t)pl.KO);
  S.s_okey = (LI32)take(4 * (size_t)pl.KO);
  S.s_ptpl = (LI32)take(4 * (size_t)pl.KO);
  S.s_phead = (LI64)take(8 * (size_t)pl.KO * R);
  S.lc.tpl = (LI32)take(4 * (size_t)pl.KL);
  S.lc.req = (LI64)take(8 * (size_t)pl.KL * R);
  S.lc.max = (LI64)take(8 * (size_t)pl.KL * R);
  S.lc.rem = (LU32)take(4 * (size_t)pl.KL * d.TW);
  S.lc.thr = (LI32)take(4 * (size_t)pl.KL * R);
  S.lc.cnt = (LI32)take(4 * (size_t)pl.KL);
  S.s_talloc = (LI64)take(TL ? 8 * (size_t)d.totalTplIts * R : 0);
  S.s_tsa = (LI64)take(TL && pl.tsort ? 8 * (size_t)d.totalTplIts * R : 0);
  S.s_tsp = (LI32)take(TL && pl.tsort ? 4 * (size_t)d.totalTplIts * R : 0);
  S.s_tbeg = (LI32)take(4 * (size_t)(d.NTPL + 1));
  S.s_pool = (LI64)take(8 * (size_t)(d.NPOOL + 1) * R);
  S.s_rs = (LU32)take(4 * (size_t)d.RSW);
  S.s_pin = (LU32)take(4 * (size_t)d.RSW);
  S.s_rem = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_cand = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_fic = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_fof = (LU32)take(4 * (size_t)d.TW + 8);
  S.s_firr = (LU32)take(4 * (size_t)d.TW + 8);
  constexpr bool MEMO = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::TPL_MEMO;
  S.s_memo = (LU32)take(MEMO ? 4 * (size_t)tpl_memo_words(R, d.TW) : 0);
  if constexpr (MEMO) S.s_memo[S.MM_T] = (uint32_t)-1;  // empty (wave-wide store of a uniform value)
  constexpr bool MASKS = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::TPL_MASKS;
  S.s_tmask = (LU32)take(MASKS && pl.tmask ? 4 * (size_t)tpl_mask_words(d.NTPL, d.TW) : 0);
  S.s_tmv = (LU32)take(MASKS && pl.tmask ? 4 * (size_t)d.NTPL : 0);
  if constexpr (MASKS) {
    if (pl.tmask)
      for (int i = lane(); i < d.NTPL; i += kWave) S.s_tmv[i] = 0;  // no row filled yet
  }
  constexpr bool CAPB = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::CAP_BOUND;
  constexpr bool CHAINB = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::RUN_CHAIN;
  constexpr bool FRONT = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::RUN_FRONT;
  S.s_fbeg = (LI32)take(FRONT ? 4 * (size_t)(d.NTPL + 1) : 0);
  S.s_front = (LI32)take(FRONT ? 4 * (size_t)D.frontTotal : 0);
  const int NWN = (d.N + 31) >> 5;
  S.s_rmv = (LU32)take(SIM ? 4 * (size_t)NWN : 0);
  S.s_tch = (LU32)take(SIM ? 4 * (size_t)NWN : 0);
  S.s_tchr = (LU32)take(SIM || d.fnOn ? 4 * (size_t)NWN : 0);
  S.s_tvol = (LU32)take(SIM ? 4 * (size_t)NWN : 0);
  S.s_vol = (LI32)take(!LEAN && d.volAny ? 4 * (size_t)Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::VO_WORDS : 0);
  if (!LEAN && d.volAny)
    for (int i = lane(); i < Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::VO_WORDS; i += kWave) S.s_vol[i] = 0;
  S.s_tgm = (LI32)take(4 * (size_t)d.G * TGM_WORDS);
  S.s_tmin = (LI32)take(4 * (size_t)d.G);
  S.s_trs0 = (LU32)take(d.G ? 4 * (size_t)d.RSW : 0);
  S.s_trs1 = (LU32)take(d.G ? 4 * (size_t)d.RSW : 0);
  S.s_tcs = (LI32)take(d.G ? 4 * (size_t)pl.tcl : 0);
  S.s_tdom = (LI32)take(4 * (size_t)pl.tdl);
  S.s_tdw = (LI32)take(SIM && TOPO ? 4 * (size_t)kTdwKeys * kTdw : 0);
  S.s_live = (LI32)take(4 * (size_t)pl.livl);
  const int NWC = SIM && d.G ? (d.tgCntWords - d.tgSmall + 31) >> 5 : 0;
  S.s_tcd = (LU32)take(4 * (size_t)NWC);
  S.s_gw = (LU64)take(TOPO && d.G && d.GMW > 1 ? 8 * (size_t)GS_N * d.GMW : 0);
  // MW: waves 1..3 hold window blocks 1..3 and serve wave 0's window steps (mw_helper); the mailbox follows
  // the plan's LDS
  constexpr bool MWK = MW && SIM && LEAN && !TOPO && RT > 0;
  const LU32 mb = (LU32)(smem + pl.lds);
  if constexpr (MWK) {
    const int wv = (int)(threadIdx.x >> 6);
    if (wv > 0) {
      mw_helper<RM>(D, W, S.s_rmv, mb, wv);
      return;
    }
  }
  if constexpr (TOPO) {  // groups in t.topologies at the start: all but the late ones (topology.go:102-119)
    if (SIM && W.tact) {  // a simulation's own: the groups its pods' starting states create (ks_cons.cpp sim_topology)
      S.t_active = W.tact[0];
      for (int w = 1 + lane(); w < d.GMW; w += kWave) S.s_gw[GS_ACT * d.GMW + w] = W.tact[w];
    } else {
      S.t_active = ~D.tg_late[0];
      for (int w = 1 + lane(); w < d.GMW; w += kWave) S.s_gw[GS_ACT * d.GMW + w] = ~D.tg_late[w];
    }
  }
  if (d.G) lds_copy<8>(S.s_tcs, D.tg_cnt0, pl.tcl);
  if (pl.tdl) lds_copy<8>(S.s_tdom, D.n_tdom, pl.tdl);
  if constexpr (SIM && TOPO) {  // the register window's node domains (Solver::tdom)
    const int nk = d.TK < kTdwKeys ? d.TK : kTdwKeys;
    for (int i = lane(); i < nk * kTdw; i += kWave) {
      const int k = i / kTdw, n = i % kTdw;
      S.s_tdw[i] = n < d.N ? D.n_tdom[(int64_t)k * d.N + n] : -1;
    }
  }
  for (int i = lane(); i < NWC; i += kWave) S.s_tcd[i] = 0;
  lds_copy<4>(S.s_tgm, D.tg_meta, d.G * TGM_WORDS);
  S.gc.tpl = W.c_tpl;
  S.gc.req = W.c_req;
  S.gc.max = W.c_max;
  S.gc.rem = W.c_rem;
  S.gc.thr = W.c_thr;
  S.gc.cnt = W.c_cnt;
  for (int i = lane(); i < d.NK * (int)(sizeof(KeyMeta) / 4); i += kWave)
    ((uint32_t KS_L*)s_keys)[i] = ((const uint32_t KS_G*)D.keys)[i];
  for (int i = lane(); i <= d.NTPL; i += kWave) S.s_tbeg[i] = D.tpl_it_beg[i];
  if constexpr (FRONT) {
    for (int i = lane(); i <= d.NTPL; i += kWave) S.s_fbeg[i] = D.tpl_front_beg[i];
    for (int i = lane(); i < D.frontTotal; i += kWave) S.s_front[i] = D.tpl_front[i];
  }
  for (int i = lane(); i < d.NPOOL * R; i += kWave) S.s_pool[i] = SIM ? W.pool0[i] : D.pool_rem0[i];
  const int P = SIM ? W.P : d.P;
  if (!SIM && d.fnOn)
    for (int i = lane(); i < NWN; i += kWave) S.s_tchr[i] = 0;
  if constexpr (SIM) {
    // the simulation's fresh Scheduler state (what k_init does for plain Solves): NewQueue order is
    // the local order (pod_map is sorted), nothing placed, no staleness marks.  The per-pod queue arrays
    // are written at the first push-back (sim_queue_init): until then nothing reads them.
    for (int i = lane(); i < NWN; i += kWave) {
      S.s_rmv[i] = 0;
      S.s_tch[i] = 0;
      S.s_tchr[i] = 0;
      S.s_tvol[i] = 0;
    }
    if constexpr (TOPO) {
      // NewTopology for this simulation: the shared counts minus the candidates' pods, which the
      // simulation schedules and NewTopology therefore excludes (topology.go:72-75,262-265); a
      // domain left with no pod and no other registration drops out of TopologyGroup.domains.
      // (copy-on-write: only the words these entries touch get a private copy)
      // placeholder counts: column 0 (the first fresh claim's); try_templates zeroes the next one per new claim
      for (int g = lane(); g < d.G; g += kWave) W.tg_ccnt[(int64_t)g * W.ccs] = 0;
      for (int i = lane(); i < d.G; i += kWave) W.tg_cpos[i] = 0;
      wsync();
      // offsets are distinct within one simulation; 4 entries per lane in flight (a long prefix has thousands)
      for (int i0 = lane(); i0 < W.ntdel; i0 += 4 * kWave) {
        int off[4], x[4], c0[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int i = i0 + u * kWave < W.ntdel ? i0 + u * kWave : i0;
          off[u] = W.tdel[2 * i];
          x[u] = W.tdel[2 * i + 1];
        }
#pragma unroll
        for (int u = 0; u < 4; u++) c0[u] = D.tg_cnt0[off[u]];
#pragma unroll
        for (int u = 0; u < 4; u++) {  // (guarded stores, no per-lane break: DESIGN §3)
          const bool live = i0 + u * kWave < W.ntdel;
          const int c = c0[u] - (x[u] >> 1);
          const int n = (c == 0 && (x[u] & 1)) ? -1 : c;
          const bool small = off[u] < d.tgSmall;
          if (live && small) S.s_tcs[off[u]] = n;
          if (live && !small) {
            W.tg_cnt[off[u]] = n;
            const int b = off[u] - d.tgSmall;
            __hip_atomic_fetch_or(S.s_tcd + (b >> 5), 1u << (b & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
          }
        }
      }
      hbm_release();
      wsync();
      for (int i = lane(); i < W.ntmd; i += kWave) S.s_tgm[W.tmd[2 * i] * TGM_WORDS + TGM_MIND] = W.tmd[2 * i + 1];
    }
    wsync();
    for (int i = lane(); i < W.nrm; i += kWave) {  // the removed candidates (a multi-node prefix: up to 101)
      const int n = W.rm[i];
      __hip_atomic_fetch_or(S.s_rmv + (n >> 5), 1u << (n & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    hbm_release();
  }
  if (TL) lds_copy<8>(S.s_talloc, D.tpl_alloc, d.totalTplIts * R);
  if (TL && pl.tsort) {
    lds_copy<8>(S.s_tsa, D.tsort_alloc, d.totalTplIts * R);
    lds_copy<8>(S.s_tsp, D.tsort_pos, d.totalTplIts * R);
  }
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

  // Register window: the first NW*64 nodes of the first-fit order (where every scan starts) stay in
  // VGPRs for the whole Solve — lane l holds nodes l, l+64, ...: taints, Available, requests and
  // flags.  A pod that fits there costs no memory round trip; commits update the owner's registers.
  constexpr int NW = RT > 0 ? 4 : 0;
  constexpr int NWA = NW > 0 ? NW : 1;
  // LEAN (no negative requests): the window keeps each node's free capacity Available - requests, so
  // Fits(requests + pod, Available) is one compare per resource; a node that can never fit (negative
  // Available, beyond N, removed by the simulation) holds INT64_MIN, which no request (>= 0) fits.
  constexpr bool FREEW = LEAN && SIM;  // (the Solve instantiations keep Available + requests: measured faster there)
  constexpr int NWQ = FREEW ? 1 : NWA;
  uint64_t wtx[NWA], wty[NWA], whp[NWA];
  int64_t wav[NWA][RM], wrq[NWQ][RM];  // FREEW: wav = free capacity, wrq unused
  int wnf[NWA];
  if constexpr (MWK) mw_barrier();  // B0a: the prologue's LDS (removed-node mask) is ready for the helpers
  if constexpr (NW > 0) {
    if (d.N > 0) {
#pragma unroll
      for (int k = 0; k < (MWK ? 1 : NW); k++) {
        const int n = k * kWave + lane(), c = n < d.N ? n : d.N - 1;
        wtx[k] = D.n_taint[2 * c];
        wty[k] = D.n_taint[2 * c + 1];
        bool never = n >= d.N;
        if (SIM) never |= S.tbit(S.s_rmv, c);
#pragma unroll
        for (int r = 0; r < RM; r++) {
          const int64_t a = D.n_avail[(int64_t)c * RM + r], q = D.n_req0[(int64_t)c * RM + r];
          if constexpr (FREEW) {
            never |= a < 0;
            wav[k][r] = a - q;
          } else {
            wav[k][r] = a;
            wrq[k][r] = q;
          }
        }
        if constexpr (FREEW)
#pragma unroll
          for (int r = 0; r < RM; r++) wav[k][r] = never ? INT64_MIN : wav[k][r];
        wnf[k] = SIM ? D.n_flags[c] : 0;
        whp[k] = D.n_hp0[c];
      }
    }
  }
  bool winUnusable = false;  // some register-window node is NF_UNUSABLE (a run's placements check it)
  if constexpr (MWK) {  // each wave's block ballot through the mailbox
    mb_st64(mb, MB_UMASK, d.N > 0 ? wballot(wnf[0] & NF_UNUSABLE) : 0ull);  // wave-wide store of a uniform value
    mw_barrier();  // B0b
#pragma unroll
    for (int q = 0; q < kMwWaves; q++) winUnusable |= mb_ld64(mb, MB_UMASK + 2 * q) != 0;
    winUnusable = ub(winUnusable);
  } else if constexpr (NW > 0) {
    if (d.N > 0)
#pragma unroll
      for (int k = 0; k < NW; k++) winUnusable |= wballot(wnf[k] & NF_UNUSABLE) != 0;
  }
  int mwseq = 0;
  // MW: post a window step to the helpers (wave-wide stores of uniform values), then B1
  auto mw_post = [&](int cmd, int m, const int64_t* fpp, uint64_t ft0, uint64_t ft1, int fpf) {
    mb[MB_M] = (uint32_t)m;
    mb[MB_FPF] = (uint32_t)fpf;
    mb_st64(mb, MB_FT0, ft0);
    mb_st64(mb, MB_FT1, ft1);
#pragma unroll
    for (int r = 0; r < RM; r++) mb_st64(mb, MB_FP + 2 * r, (uint64_t)fpp[r]);
    mb[MB_SEQ] = (uint32_t)++mwseq;
    mb[MB_CMD] = (uint32_t)cmd;
    mw_barrier();  // B1
  };
  // MW: block 0's first-fit ballot, then every block's (B2); returns the first block holding a fit
  auto mw_fit = [&](const int64_t* fpp, uint64_t ft0, uint64_t ft1, uint64_t& mj) {
    mw_post(MW_FIT, 0, fpp, ft0, ft1, 0);
    bool ok = (((wtx[0] & ~ft0) | (wty[0] & ~ft1)) == 0);
#pragma unroll
    for (int r = 0; r < RM; r++) ok &= fpp[r] <= wav[0][r];
    mb_st64(mb, MB_MASK, wballot(ok));
    mw_barrier();  // B2
    return mw_first_fit(mb, mj);
  };
  int nclaims = 0, nlog = 0, hostCtr = SIM ? 0 : d.hostnameSeed;
  bool allSched = true;  // SIM: AllNonPendingPodsScheduled so far (pods placed on unusable nodes)
  int nrs = 0;           // SIM: compact node-requirement slots in use
  bool srt = true;      // s.newNodeClaims non-decreasing in len(Pods)
  // the sorted position whose count increment left the pending descent (!srt); -1: an appended claim, or not
  // tracked (sort_claims' closed form, KS_SORT_CLOSED)
  constexpr bool SORTC = Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::SORT_CLOSED;
  int dpos = -1;
  bool dapp = false;  // ... and that it is an appended claim's (try_templates left it)
  int64_t sortsClosed = 0;
  bool pushed = false;  // a failed pod was pushed back since the last window refill
  // no pod was pushed back yet (refill reads the pods' first states directly); a probe re-run from carried pods
  // starts with its queue state written (its pods' starting states are not all the first ones)
  bool ident = !(SIM && W.sstart);
  bool anyRelaxed = false;  // SIM: some Preferences.Relax changed a pod (the record's RB_RELAXED)
  uint32_t epoch = 1;
  int qhead = 0, qlen = P;
  if (SIM && !ident) S.sim_queue_init(P);
  int wn = 0, wi = 0;  // window size / next index
  int64_t pops = 0, sorts = 0, slow = 0, exact = 0, windows = 0, fulls = 0, fullFails = 0, runs = 0, runPods = 0;
  // LEAN Solve claim runs across re-sorts (KS_RUN_CROSS): crossings continued inside a step, continuations refused
  // (a position before the claim's new one passed the quick test), and the refusals after which the pod landed
  // on the run's claim all the same (the only ones that cost a step: any other ends the run anyway)
  int64_t cross = 0, crossStops = 0, crossLost = 0;
  // ... in-run re-sorts that took the closed form, and moves of a run's claim in the position arrays (KS_RUN_FUSE)
  int64_t crossClosed = 0, runMoves = 0;
  int stopC = -1;                    // the claim of a continuation just refused
  int64_t sortB = 0, pendSortB = 0;  // this add()'s re-sort bytes; those of a re-sort run for the next add()
  // LEAN Solve (KS_RUN_CHAIN): the pod just placed landed on a NodeClaim and the next queue pod is identical to it
  // (the claim runs' identity): that pod's step skips the node phase.  The identical pod before it failed every
  // existing node, a LEAN pod has no host ports, volumes or keys, and nodes only change when a pod lands on one:
  // none did.  nodeAB: the node phase's algorithmic bytes of the last pod that ran it, credited to each chained pod
  bool chain = false;
  int64_t nodeAB = 0, chainPods = 0;
  // Every pop either places a pod, relaxes it, or marks it stale; the reference's queue can cycle
  // O(P^2) in adversarial inputs, far beyond any realistic batch.  Bound it so a logic error ends the
  // kernel with KE_ITER_CAP instead of hanging the device.
  const int64_t popCap = (int64_t)64 * (d.S + P) + 100000;
  int err = KE_OK;
  Window<RT> w;
  int64_t pod[RM];
  int64_t req[RM];
  int nthr[RM];
  // TOPO Solve: nodes [0, rskip) fail Fits for the last popped request vector.  Requests on a node only grow, so
  // a following pod with the same requests fails them too and its first-fit scan starts at rskip (the first
  // fit is unchanged: only nodes failing the resource test are passed over).
  // (Solves only: the topology simulations measured slower with it, C5 + topology 11.65 ms against 10.92 ms)
  constexpr bool RSK = TOPO && !SIM;
  int rskip = 0;
  int64_t prqv = 0;  // lane r: request r of the last popped pod
  // Solve: the live node list.  The existing nodes past the register window that pass Fits for the popped
  // request vector, in first-fit order (S.s_live; -1 marks a node a commit has filled).  Requests on a node
  // only grow, so within a run of pods with identical requests a node failing Fits fails it for good; the
  // first-fit scan walks the list and never loads such a node again (the first fit is unchanged: only
  // nodes failing the resource test are left out).  Rebuilt when the request vector changes.
  constexpr bool LIVE = !SIM && !LEAN && NW > 0;
  const bool liveOn = LIVE && pl.livl > 0;
#ifndef KS_LIVE_ALL
#define KS_LIVE_ALL 1
#endif
  // The list also covers the register window's nodes, which are then not scanned from registers: a window
  // whose nodes pass Fits but fail the pod's other tests cost every pod its topology tests there (C4: 139k ->
  // 151k pods/s with the window in the list, profiles/r05_la_c4_*.json; KS_LIVE_ALL=0 keeps the window)
  const bool liveAll = KS_LIVE_ALL && liveOn && d.N > NW * kWave;
  bool liveOK = false;
  int nlive = 0, lstart = 0;  // list entries [0, lstart) are all -1 (first-fit fills the list from its front)
#ifdef KS_PHASE_STATS
  uint64_t cyc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  uint64_t fcyc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t tstart = __builtin_amdgcn_s_memtime();
#endif

  while (true) {
    qlen = UI(qlen);
    qhead = UI(qhead);
    wi = UI(wi);
    wn = UI(wn);
    if (qlen <= 0) break;
    PH_BEGIN(t0);
    if (wi == wn) {
      PH_BEGIN(tr);
      S.refill(w, qhead, qlen, P, pushed, ident);
      FPH_END(tr, 2);
      if (FREEW) SPHS_END(S, tr, 0);  // simulation fast path (stats build): window refills
      pushed = false;
      wn = qlen < kWave ? qlen : kWave;
      wi = 0;
      windows++;
    }
    if constexpr (FREEW && NW > 0) {
      // Fast path of a simulation over resource-only pods (what consolidation re-schedules): while the
      // next pops each fit a node of the register window, the step is Queue.Pop + the window's
      // first-fit ballots + the commit to the owner lane's registers, with nothing else live.  A pod
      // that fits no window node (or a stale queue) leaves it un-popped for the general step below.
      // (A simulation's placements are not read back -- its record is -- so nothing is logged here.  SLOG, the
      // re-run whose placements are: every pod takes the single-pod step below, which logs it; a run places its
      // pods on the same nodes in the same order, so the record is the same.)
      if (d.N > 0) {
        while (wi < wn) {
          const uint64_t fll = (uint64_t)rdl64((int64_t)w.ll, wi);
          if ((uint32_t)(fll >> 32) == epoch && (uint32_t)fll == (uint32_t)qlen) break;
          const uint64_t ft0 = (uint64_t)rdl64((int64_t)w.tol0, wi), ft1 = (uint64_t)rdl64((int64_t)w.tol1, wi);
          const int fpf = rdl(w.pf, wi);
          int64_t fp[RM];
#pragma unroll
          for (int r = 0; r < RM; r++) fp[r] = rdl64(w.req[r], wi);
          // A run of identical pods (same requests, tolerations and provisionable flag, none stale when it is
          // popped): pod after pod, first-fit fills the window's nodes in order, each taking as many as fit (min
          // over resources of floor(free / request)), so the whole run is placed in one step -- per node its
          // capacity for the run, an exclusive scan over the node order, each node's share.  While no pod was
          // pushed back (ident) the queue is the NewQueue order and the run is k_sim_run_len's count at this
          // position, which may reach past the window; otherwise the identical, non-stale pods that follow in
          // the window.
          int m;
          if (ident) {
            m = rdl(w.rl, wi);
            m = m < qlen ? m : qlen;
          } else {
            bool inrun = false;
            if (lane() >= wi && lane() < wn) {
              bool same = w.tol0 == ft0 && w.tol1 == ft1 && ((w.pf ^ fpf) & PF_PROVISIONABLE) == 0;
#pragma unroll
              for (int r = 0; r < RM; r++) same &= w.req[r] == fp[r];
              const uint32_t qx = (uint32_t)(qlen - (lane() - wi));
              inrun = same && !((uint32_t)(w.ll >> 32) == epoch && (uint32_t)w.ll == qx);
            }
            const uint64_t nr = wballot(!inrun) & (~0ull << wi);
            m = (nr ? ctz64(nr) : kWave) - wi;
          }
          m = uni(m);
          if (!SLOG && m >= KS_RUN_MIN) {
            PH_BEGIN(tb);
            float rq[RM];
#pragma unroll
            for (int r = 0; r < RM; r++) rq[r] = run_rcp(fp[r]);
            int placed = 0;
            bool unusable = false;
            int ab = 0;  // sum over the run's pods of their node's position + 1 (< 2^31 below 8M pods per run)
            if constexpr (MWK) {
              // block 0 here, blocks 1..3 on the helpers; the blocks' totals give each its base
              mw_post(MW_RUN, m, fp, ft0, ft1, fpf);
              const bool tol = (((wtx[0] & ~ft0) | (wty[0] & ~ft1)) == 0);
              int cap = tol ? m : 0;
#pragma unroll
              for (int r = 0; r < RM; r++) {
                const int c = run_cap(wav[0][r], fp[r], rq[r], m);
                cap = c < cap ? c : cap;
              }
              const int incl = wscan_add(cap);
              mb[MB_TOT] = (uint32_t)rdl(incl, kWave - 1);  // wave-wide store of a uniform value
              mw_barrier();  // B2
              int tot = 0;
#pragma unroll
              for (int q = 0; q < kMwWaves; q++) tot += (int)mb[MB_TOT + q];
              tot = uni(tot);
              placed = tot < m ? tot : m;
              // (placed == 0: every block's capacity is 0, so every share below is 0)
              const int p0 = incl - cap, room = m - p0;
              const int tk0 = room <= 0 ? 0 : (cap < room ? cap : room);
#pragma unroll
              for (int r = 0; r < RM; r++) wav[0][r] -= (int64_t)tk0 * fp[r];
              unusable = tk0 > 0 && (wnf[0] & NF_UNUSABLE);
              ab = tk0 * (lane() + 1);
              if (placed == 0) break;  // pod wi fits no window node: the general step
            } else {
              int tk[NWA];
              int base = 0, nb = 0;  // nb: the window blocks the run reaches (the rest take nothing)
#pragma unroll
              for (int k = 0; k < NW; k++) {
                tk[k] = 0;
                if (base < m) {
                  nb = k + 1;
                  const bool tol = (((wtx[k] & ~ft0) | (wty[k] & ~ft1)) == 0);
                  int cap = tol ? m : 0;
#pragma unroll
                  for (int r = 0; r < RM; r++) {
                    const int c = run_cap(wav[k][r], fp[r], rq[r], m);
                    cap = c < cap ? c : cap;
                  }
                  const int incl = wscan_add(cap);
                  const int p0 = base + incl - cap, room = m - p0;
                  tk[k] = room <= 0 ? 0 : (cap < room ? cap : room);
                  base += rdl(incl, kWave - 1);
                }
              }
              placed = base < m ? base : m;
              if (placed == 0) break;  // pod wi fits no window node: the general step
              // commit: each node's share, in the blocks the run reached (branch-free per lane: tk = 0 leaves a
              // node unchanged)
#pragma unroll
              for (int k = 0; k < NW; k++) {
                if (k < nb) {
#pragma unroll
                  for (int r = 0; r < RM; r++) wav[k][r] -= (int64_t)tk[k] * fp[r];
                  unusable = unusable || (tk[k] > 0 && (wnf[k] & NF_UNUSABLE));
                  ab += tk[k] * (k * kWave + lane() + 1);
                }
              }
            }
            // AllNonPendingPodsScheduled: a non-provisionable pod on an unusable node (helpers.go:118-124)
            if (winUnusable && !(fpf & PF_PROVISIONABLE) && wballot(unusable)) allSched = false;
            // a run's pods within the window that had failed before (only after a push-back) are scheduled now
            if (!ident && lane() >= wi && lane() < wi + placed && lane() < wn && w.st == ST_FAILED)
              W.pod_status[w.p] = ST_SCHEDULED;
            S.algbytes += (int64_t)rdl(wscan_add(ab), kWave - 1) * (16 * R + 16);
            nlog += placed;
            qhead += placed;
            if (qhead >= P) qhead -= P;
            qlen -= placed;
            pops += placed;
            wi += placed;
            if (wi > wn) wi = wn;  // the run reached past the window: refill at the loop head
            runs++;
            runPods += placed;
            SPHS_END(S, tb, 1);  // (stats build): runs placed in one step
            if (placed < m) break;  // the next pod of the run fits no window node
            continue;
          }
          int kj = -1;
          uint64_t mj = 0;
          if constexpr (MWK) {
            kj = mw_fit(fp, ft0, ft1, mj);
          } else {
#pragma unroll
            for (int k = 0; k < NW; k++) {
              bool ok = (((wtx[k] & ~ft0) | (wty[k] & ~ft1)) == 0);
#pragma unroll
              for (int r = 0; r < RM; r++) ok &= fp[r] <= wav[k][r];
              const uint64_t m = wballot(ok);
              if (m) {
                kj = k;
                mj = m;
                break;
              }
            }
          }
          if (kj < 0) break;
          const int fpod = rdl(w.p, wi);
          const int j = kj * kWave + ctz64(mj), owner = j & (kWave - 1);
          int nfv = 0;
          if constexpr (MWK) {  // block 0 commits here, the helper owning block kj commits there
            const bool own = kj == 0 && lane() == owner;
#pragma unroll
            for (int r = 0; r < RM; r++) wav[0][r] -= own ? fp[r] : 0;
            nfv = ((mb_ld64(mb, MB_UMASK + 2 * kj) >> owner) & 1ull) ? NF_UNUSABLE : 0;
          } else {
#pragma unroll
            for (int k = 0; k < NW; k++)
              if (k == kj) {
                nfv = wnf[k];
                if (lane() == owner)
#pragma unroll
                  for (int r = 0; r < RM; r++) wav[k][r] -= fp[r];
              }
          }
          if ((rdl(nfv, owner) & NF_UNUSABLE) && !(fpf & PF_PROVISIONABLE)) allSched = false;
          if (rdl(w.st, wi) == ST_FAILED) W.pod_status[fpod] = ST_SCHEDULED;  // (wave-wide, uniform)
          if constexpr (SLOG) S.log_commit(fpod, -(j + 1), nlog);
          else nlog++;
          S.algbytes += (int64_t)(j + 1) * (16 * R + 16);
          qhead = qhead + 1 == P ? 0 : qhead + 1;
          qlen--;
          pops++;
          wi++;
        }
        if (wi == wn) continue;  // window drained: refill (or finish) at the loop head
      }
    }
    // Queue.Pop (queue.go:46-61)
    const int p = rdl(w.p, wi);
    const int g = SIM ? rdl(w.g, wi) : p;
    const int uid = rdl(w.uid, wi);
    uint64_t ll = (uint64_t)rdl64((int64_t)w.ll, wi);
    if (S.dupU()) {
      hbm_release();
      ll = uni64((int64_t)ld_sc1(W.last_len + uid));
    }
    if (U((uint32_t)(ll >> 32) == epoch && (uint32_t)ll == (uint32_t)qlen)) break;
    qhead = qhead + 1 == P ? 0 : qhead + 1;
    qlen--;
    if (++pops > popCap) { err = KE_ITER_CAP; break; }
    const int64_t abPop = S.algbytes;  // (claim runs: one pod's algorithmic bytes)
    const int prevStop = stopC;        // (claim runs: the claim whose run the step before left to this pod's scan)
    stopC = -1;
    // KS_RUN_CHAIN: a chained pod is a popped pod (`pops` counts it, `runPods` does not); its run length is kept for
    // the chain test at the step's end
    const bool chained = CHAINB && chain;
    const int rlp = CHAINB ? rdl(w.rl, wi) : 0;
    if constexpr (CHAINB) {
      chain = false;
      chainPods += chained;
    }
    const int s = rdl(w.s, wi);
    const int sflags = rdl(w.flags, wi);
    const uint64_t toltpl = (uint64_t)rdl64((int64_t)w.toltpl, wi);
    const uint64_t tol0 = (uint64_t)rdl64((int64_t)w.tol0, wi), tol1 = (uint64_t)rdl64((int64_t)w.tol1, wi);
    if (S.hpA()) {
      S.cur_hpc = (uint64_t)rdl64((int64_t)w.hpc, wi);
      S.cur_hpu = (uint64_t)rdl64((int64_t)w.hpu, wi);
      S.cur_hpo = (uint64_t)rdl64((int64_t)w.hpo, wi);
    }
    const int pfl = S.volA() ? rdl(w.pf, wi) : 0;
    if (S.volA()) S.vol_pop(g, pfl);
    PH_BEGIN(tst);
    if (S.keys(sflags)) {  // the state's record, read by every check of this pop
      S.copy_words(S.s_pin, D.st_rs + (int64_t)s * d.RSW, d.RSW);
      S.fnp = d.fnOn ? D.st_fn + (int64_t)uni(D.st_fnrow[s]) * ((d.N + 31) >> 5) : nullptr;
      wsync();
    }
    FPH_END(tst, 1);
    PH_BEGIN(ttpop);
    if (TOPO)
      S.topo_pop(s, SIM ? rdl(w.g, wi) : rdl(w.p, wi), (uint64_t)rdl64((int64_t)w.tsel, wi),
                 (uint64_t)rdl64((int64_t)w.tinv, wi), (uint64_t)rdl64((int64_t)w.town, wi),
                 (uint64_t)rdl64((int64_t)w.trss, wi));
    FPH_END(ttpop, 0);
#pragma unroll
    for (int r = 0; r < RM; r++) {
      if (RT == 0 && r >= R) break;
      pod[r] = rdl64(w.req[r], wi);
    }
    wi++;
    if (RSK || liveOn) {
      int64_t mine = 0;
#pragma unroll
      for (int r = 0; r < RM; r++) {
        if (RT == 0 && r >= R) break;
        mine = lane() == r ? pod[r] : mine;
      }
      const bool differ = wballot(lane() < R && mine != prqv) != 0;
      if (RSK) rskip = differ || d.tgUnlab || d.negReq ? 0 : rskip;  // (a negative request can free capacity)
      liveOK = liveOK && !differ;
      prqv = mine;
    }
    PH_END(t0, 0);
    bool placed = false;
    bool onClaim = false;  // KS_RUN_CHAIN: the pod landed on a NodeClaim (claim scan or try_templates) ...
    int kRun = 0;          // ... and the run that followed placed this many more
#ifdef KS_PHASE_STATS
    int skind = KD_CYC_SINGLE;  // the step's kind (KindSub): a single pod unless it opens a NodeClaim or places a run
#endif
    int rfirst = -1;  // RSK: the first node of this scan passing the resource test (-1: none yet)
    // 1) existing nodes in order (none can pass when a matching group admits no domain)
    PH_BEGIN(t1);
    // (unlabelled nodes choose their domain from their requirements: no shortcut then)
    // (GetVolumes failing for the pod fails ExistingNode.Add on every node, existingnode.go:70-73)
    // (KS_RUN_CHAIN: every node failed the identical pod before this one and none changed since)
    const bool skipNodes = (TOPO && S.t_nonode && !d.tgUnlab) || (S.volA() && (pfl & PF_VOLERR)) || chained;
    const int64_t abNode = CHAINB ? S.algbytes : 0;
    int scanFrom = 0;
    if constexpr (NW > 0) {
      // (problems with unlabelled nodes scan every node through node_okK, which handles them)
      if (d.N > 0 && !skipNodes && !(TOPO && d.tgUnlab) && !liveAll) {
        int kj = -1;
        uint64_t mj = 0;
        asm volatile("; KS_MARK window_begin");
        PH_BEGIN(twin);
        if constexpr (MWK) kj = mw_fit(pod, tol0, tol1, mj);  // (LEAN: no host ports, volumes, keys)
#pragma unroll
        for (int k = 0; k < (MWK ? 0 : NW); k++) {
          if (RSK && (k + 1) * kWave <= rskip) continue;  // every node of the block fails Fits
          const int n = k * kWave + lane();
          bool rok = true;  // in range, not removed, Fits: permanent failures for these requests
          if constexpr (FREEW) {
#pragma unroll
            for (int r = 0; r < RM; r++) rok &= pod[r] <= wav[k][r];
          } else {
            rok &= n < d.N;
            if (SIM) rok &= !S.tbit(S.s_rmv, n < d.N ? n : 0);
#pragma unroll
            for (int r = 0; r < RM; r++) rok &= (wav[k][r] >= 0) & (wrq[k][r] + pod[r] <= wav[k][r]);
          }
          if constexpr (RSK) {
            const uint64_t rm = wballot(rok);
            rfirst = rfirst < 0 && rm ? k * kWave + ctz64(rm) : rfirst;
          }
          bool ok = rok & (((wtx[k] & ~tol0) | (wty[k] & ~tol1)) == 0);
          ok &= (whp[k] & S.cur_hpc) == 0;
          if (S.volA() && S.vol_any() && ok) ok = S.vol_ok(n);
          if (S.keys(sflags) && ok) ok = S.node_compat(n);
          PH_BEGIN(twt);
          if (TOPO && S.t_any && ok) {  // every node is labelled here
            int cn = n < d.N ? n : d.N - 1;
            bool sl;
            S.template topo_node_stateK<1>(&cn, &ok, &sl);
          }
          FPH_END(twt, 7);
#ifdef KS_PHASE_STATS
          fcyc[4] += 1;
#endif
          const uint64_t m = wballot(ok);
          if (m) {
            kj = k;
            mj = m;
            break;
          }
        }
        asm volatile("; KS_MARK window_end");
        FPH_END(twin, 3);
        if (U(kj >= 0)) {
          const int j = kj * kWave + ctz64(mj), owner = j & (kWave - 1);
          int nfv = 0;
          if constexpr (MWK) {
            const bool own = kj == 0 && lane() == owner;
#pragma unroll
            for (int r = 0; r < RM; r++) wav[0][r] -= own ? pod[r] : 0;
            nfv = ((mb_ld64(mb, MB_UMASK + 2 * kj) >> owner) & 1ull) ? NF_UNUSABLE : 0;
          }
#pragma unroll
          for (int k = 0; k < (MWK ? 0 : NW); k++)
            if (k == kj) {
              nfv = wnf[k];
              if (lane() == owner) {
#pragma unroll
                for (int r = 0; r < RM; r++) {
                  if constexpr (FREEW) wav[k][r] -= pod[r];
                  else wrq[k][r] += pod[r];
                }
                whp[k] = (whp[k] & ~S.cur_hpo) | S.cur_hpu;
              }
            }
          if (S.volA() && S.vol_any()) S.vol_commit(j);
          PH_BEGIN(t7);
          if constexpr (SIM) {
            PH_BEGIN(tnc);
            if (S.keys(sflags)) S.sim_node_commit(j, s, sflags, pod, pod, nrs, true);
            FPH_END(tnc, 6);
            if ((rdl(nfv, owner) & NF_UNUSABLE) && !(rdl(w.pf, wi - 1) & PF_PROVISIONABLE)) allSched = false;
          } else if (S.keys(sflags) && lane() == owner) {
            rs_add(S.L, W.n_rs + (int64_t)j * d.RSW, S.s_pin);
            S.node_rs_changed(j);
          }
          PH_BEGIN(trec);
          if (TOPO && S.t_rec) S.topo_record(S.node_rs(j), -1, j, 0, nlog);  // existingnode.go:121
          FPH_END(trec, 5);
          S.log_commit(p, -(j + 1), nlog);
          PH_END(t7, 7);
          S.algbytes += (int64_t)(j + 1) * (16 * R + 16);
          placed = true;
        } else {
          S.algbytes += (int64_t)min(NW * kWave, d.N) * (16 * R + 16);
        }
        scanFrom = NW * kWave;
      }
    }
    const bool useLive = liveOn && !skipNodes && d.N > scanFrom;
    SPHS_END(S, t1, 0);  // stats build: the node phase up to the scan past the register window
    PH_BEGIN(tlb);
    if (useLive && !U(liveOK)) {  // the list for this request vector: every node past the window passing Fits
      wsync();
      int cnt = 0;
      for (int base = scanFrom; base < d.N; base += kWave) {
        const int n = base + lane(), c = n < d.N ? n : d.N - 1;
        bool rok = n < d.N;
#pragma unroll
        for (int r = 0; r < RM; r++) {
          if (RT == 0 && r >= R) break;
          const int64_t a = D.n_avail[(int64_t)c * R + r], q = W.n_req[(int64_t)c * R + r];
          rok &= (a >= 0) & (q + pod[r] <= a);
        }
        const uint64_t m = wballot(rok);
        if (rok) S.s_live[cnt + popc64(m & ((1ull << lane()) - 1))] = n;
        cnt += popc64(m);
      }
      nlive = UI(cnt);
      lstart = 0;
      liveOK = true;
      wsync();
    }
    PH_BEGIN(tls);
    const int scanEnd = useLive ? nlive : d.N;
    int jpos = -1;  // useLive: the list position of the fit
    for (int base = skipNodes ? scanEnd : useLive ? lstart : (RSK && rskip > scanFrom ? rskip : scanFrom); U(base < scanEnd && !placed);
         base += KS_NODE_K * kWave) {
      constexpr int KN = KS_NODE_K;
#ifdef KS_PHASE_STATS
      S.scyc[2] += 1;  // scan steps past the window
#endif
      bool ok[KN], sl[KN], rk[KN], stay[KN];
      int nf[KN];
      int64_t q[KN][RM];
      if (useLive) {
        int nl[KN];
#pragma unroll
        for (int i = 0; i < KN; i++) {
          const int pos = base + i * kWave + lane();
          nl[i] = pos < nlive ? S.s_live[pos] : -1;
        }
        S.template node_okK<KN, true>(0, sflags, pod, tol0, tol1, ok, nf, q, sl, rk, nl, stay);
      } else {
        S.template node_okK<KN>(base + lane(), sflags, pod, tol0, tol1, ok, nf, q, sl, rk);
        if constexpr (RSK) {
#pragma unroll
          for (int i = 0; i < KN; i++) {
            const uint64_t rm = wballot(rk[i]);
            rfirst = rfirst < 0 && rm ? base + i * kWave + ctz64(rm) : rfirst;
          }
        }
      }
      uint64_t mk[KN];
#pragma unroll
      for (int i = 0; i < KN; i++) mk[i] = wballot(ok[i]);
      int j = -1;
      bool slowj = false;
#pragma unroll
      for (int i = KN - 1; i >= 0; i--)
        if (mk[i]) j = base + i * kWave + ctz64(mk[i]);
      if (useLive && j >= 0) {  // list position -> node; the list keeps the node while it still fits
        jpos = UI(j);
        const int hi = (jpos - base) >> 6, owner = (jpos - base) & (kWave - 1);  // (base: any list position)
        bool st = false;
#pragma unroll
        for (int i = 0; i < KN; i++)
          if (i == hi) st = stay[i];
        st = rdl((int)st, owner) != 0;
        j = S.s_live[jpos];
        if (!st) S.s_live[jpos] = -1;  // wave-wide store of a uniform value
        j = UI(j);
        if (!st && jpos == lstart) {  // the front moves past the filled entries
          lstart++;
          while (U(lstart < nlive)) {
            const int pos = lstart + lane();
            const uint64_t m = wballot(pos >= nlive || S.s_live[pos] >= 0);
            if (m) {
              lstart += ctz64(m);
              break;
            }
            lstart += kWave;
          }
          lstart = UI(lstart < nlive ? lstart : nlive);
        }
      }
      if (TOPO && d.tgUnlab) {  // unlabelled nodes before the first fast fit are decided wave-wide, in order
#pragma unroll
        for (int i = 0; i < KN; i++) {
          if (slowj) break;
          uint64_t sm = wballot(sl[i]);
          const uint64_t fm = mk[i];
          if (fm) sm &= (fm & (~fm + 1)) - 1;  // only those before this block's first fast fit
          for (; sm && !slowj; sm &= sm - 1) {
            const int jj = base + i * kWave + ctz64(sm);
            if (S.node_slow(jj, s, sflags)) {
              j = jj;
              slowj = true;
            }
          }
          if (fm) break;
        }
      }
      j = UI(j);
      if (j >= 0) {
        const int hi = ((useLive ? jpos : j) - base) >> 6;  // the block of the step holding node j
        S.algbytes += (int64_t)(j - (useLive ? scanFrom : base) + 1) * (16 * R + 16);
        PH_BEGIN(t7);
        if (S.volA() && S.vol_any()) S.vol_commit(j);
        const int fl = slowj ? (sflags & ~SF_HAS_KEYS) : sflags;  // node_slow's record replaces rs_add
        if constexpr (SIM) {
          int64_t qs[RM];
          int nfs = 0;
#pragma unroll
          for (int i = 0; i < KN; i++)
            if (i == hi) {
              nfs = nf[i];
#pragma unroll
              for (int r = 0; r < RM; r++) qs[r] = q[i][r];
            }
          S.sim_node_commit(j, s, fl, pod, qs, nrs, false);
          const int nfj = rdl(nfs, j & (kWave - 1));
          if ((nfj & NF_UNUSABLE) && !(rdl(w.pf, wi - 1) & PF_PROVISIONABLE)) allSched = false;
        } else if (lane() == (j & (kWave - 1))) {
          S.node_commit(j, s, fl, pod);  // the owner lane of node j
        }
        if (TOPO && slowj) {
          S.node_store_rs(j, nrs);
          if (S.t_rec) S.topo_record(S.s_rs, -1, -1, 0, nlog);  // existingnode.go:121
        } else if (TOPO && S.t_rec) {
          S.topo_record(S.node_rs(j), -1, j, 0, nlog);  // existingnode.go:121
        }
        S.log_commit(p, -(j + 1), nlog);
        PH_END(t7, 7);
        placed = true;
      } else if (!useLive) {
        S.algbytes += (int64_t)min(KN * kWave, d.N - base) * (16 * R + 16);
      }
    }
    if (useLive && !placed) S.algbytes += (int64_t)(d.N - scanFrom) * (16 * R + 16);
    SPHS_END(S, tls, 3);  // stats build: the scan past the window
    PH_END(t1, 1);
    if constexpr (CHAINB) {  // the skipped node phase counts what it counted for the identical pod that ran it
      if (chained) S.algbytes += nodeAB;
      else if (!placed) nodeAB = S.algbytes - abNode;
    }
    // every node from rskip on was tested (up to the fit, if any): the first passing Fits bounds the prefix
    // (with the live list the scan past the window tested only live nodes: the window's prefix is what is known)
    if (RSK && !skipNodes && d.N > 0) rskip = rfirst >= 0 ? rfirst : useLive ? scanFrom : d.N;
    // A simulation's pod one of whose (non-hostname) groups admits no domain at all (t_nonode) fails every
    // NodeClaim too: the claims' domain choices are a subset of the domains topo_pop already found empty
    // (nextDomainTopologySpread / Affinity / AntiAffinity over fewer values), and a failed topo_apply has no
    // side effect.  Simulations render no messages, so only the NewNodeClaim calls are counted (the
    // record's RF_HOSTINCR).  The claim re-sort of this add() still runs: s.newNodeClaims' order after the last
    // add() is what NewNodeClaims[0] of the record reads.
    const bool simNoClaim = SIM && TOPO && S.t_nonode && d.NTPL > 0;
    // 2) in-flight NodeClaims, sorted by pod count
    if (U(!placed && nclaims > 0)) {
      PH_BEGIN(t2);
      sorts++;
      sortB = pendSortB;  // a re-sort the step before ran for this add() (KS_RUN_CROSS, a refused continuation)
      S.algbytes += pendSortB;
      pendSortB = 0;
      if (!U(srt)) {
        const int64_t ab = S.algbytes;
        int npos;
        const int how = S.sort_claims(nclaims, SORTC ? dpos : -1, npos, SORTC && dapp);
        exact += how == S.SORT_EXACT;
        sortsClosed += how == S.SORT_CLOSED_FORM;
        slow++;
        srt = true;
        dpos = -1;
        dapp = false;
        sortB += S.algbytes - ab;
      }
      PH_END(t2, 2);
      int stepFF = 0;  // positions of this scan that passed the quick test and failed claim_full
      for (int base = 0; U(base < nclaims && !placed && !simNoClaim); base += kWave) {
        PH_BEGIN(t3);
        const int j = base + lane();
        const bool q = j < nclaims && S.claim_quick(j, s, sflags, toltpl, pod);
        uint64_t m = wballot(q);
        S.algbytes += (int64_t)min(kWave, nclaims - base) * (8 * R + 4);
        PH_END(t3, 3);
        while (U(m != 0 && !placed)) {
          const int jj = base + ctz64(m);
          m &= m - 1;
          const int c = uni(S.s_order[jj]);
          PH_BEGIN(t4);
          const bool inl = c < pl.KL;
          int ncnt = 0;
          const bool ok = U(inl ? S.template claim_full<true>(c, s, sflags, pod, req, nthr, ncnt)
                                 : S.template claim_full<false>(c, s, sflags, pod, req, nthr, ncnt));
          fulls++;
          PH_END(t4, 4);
          PH_BEGIN(t5);
          if (ok) {
            srt = U(inl ? S.template commit_claim<true>(c, jj, nclaims, p, sflags, pod, req, nthr, ncnt, nlog)
                         : S.template commit_claim<false>(c, jj, nclaims, p, sflags, pod, req, nthr, ncnt, nlog));
            placed = true;
            if constexpr (CHAINB) onClaim = true;
            if constexpr (SORTC) dpos = srt ? -1 : jj;
            if constexpr (LEAN && !SIM && KS_CLAIM_RUNS) {
              // the identical pods that follow land here too (claim_run_cap): placed in one step.  While nothing
              // was pushed back (ident) the queue is NewQueue's order and the run is the popped pod's run length
              // (launch_solve's sim_run_lengths), which may reach past the window; otherwise the identical,
              // non-stale pods that follow in the window.
              // (KS_RUN_CROSS: a commit that left a descent enters too -- the run starts with the re-sort)
              if (KS_RUN_CROSS && prevStop == c) crossLost++;  // the refused pod landed on the run's claim after all
              if ((srt || KS_RUN_CROSS) && (ident || wi < wn)) {
                int m;
                if (ident) {
                  m = rdl(w.rl, wi - 1) - 1;
                  m = m < qlen ? m : qlen;
                } else {
                  bool inrun = false;
                  if (lane() >= wi && lane() < wn) {
                    bool same = w.toltpl == toltpl && w.tol0 == tol0 && w.tol1 == tol1;
#pragma unroll
                    for (int r = 0; r < RM; r++) {
                      if (RT == 0 && r >= R) break;
                      same &= w.req[r] == pod[r];
                    }
                    const uint32_t qx = (uint32_t)(qlen - (lane() - wi));
                    inrun = same && !((uint32_t)(w.ll >> 32) == epoch && (uint32_t)w.ll == qx);
                  }
                  const uint64_t nr = wballot(!inrun) & (~0ull << wi);
                  m = (nr ? ctz64(nr) : kWave) - wi;
                }
                m = UI(m);
                if (m > 0) {
                  int pos = jj, k;
                  int64_t credit;  // the run pods' algorithmic bytes
                  const int64_t ab0 = S.algbytes;
                  if constexpr (KS_RUN_CROSS) {
                    // The run stays on its claim across re-sorts.  Its capacity for this pod is taken once; each
                    // segment runs to the pod that lifts the claim's count past the next position's, where the
                    // next add() would re-sort: the descent's count is stored and sort_claims runs as it would
                    // there.  The run goes on at the claim's new position p' while every position before p' fails
                    // the quick test (an upper bound, so a certain reject; those claims did not change in this
                    // step).  One that passes stops it: the array is sorted and the next pod takes its own step.
                    PH_BEGIN(trc);
                    int cap = 0;
                    if (CAPB && S.capOver) {
                      S.capBoundSkips++;  // KS_CAP_BOUND: no option takes a second pod
                    } else {
                      cap = inl ? S.template claim_run_cap<true>(c, pod, m) : S.template claim_run_cap<false>(c, pod, m);
#ifdef KS_PHASE_STATS
                      S.kcyc[KD_CAP_ZERO] += cap == 0;  // (calls made only: a skipped call is capBoundSkips')
#endif
                    }
                    SXPH_END(S, trc, SS_RUN_CAP);
                    PH_BEGIN(tcl);
                    int left = m < cap ? m : cap, K = uni(S.s_okey[jj]);
                    // a segment's pods are credited with the first pod's span, the re-sort's regather and the
                    // quick-scan chunks swapped for the segment's own
                    const int64_t qbytes = 8 * R + 4;
                    const int64_t span0 = ab0 - abPop - sortB - (int64_t)min((jj / kWave + 1) * kWave, nclaims) * qbytes;
                    int64_t per = ab0 - abPop;
                    k = 0;
                    credit = 0;
                    if constexpr (KS_RUN_FUSE && SORTC) {
                      // KS_RUN_FUSE: the position arrays stay untouched while the run advances.  The claim's entry
                      // stays at pos0; the array the next add() would see has it at p with count K and the entries
                      // between one place to the left (Solver::run_materialise makes it so: at a stop, before a
                      // general re-sort, at the run's end).  A crossing is closed-form under sort_claims' conditions,
                      // choosePivot's hint read on that array (w_choose_pivot_moved); it lifts the claim over the
                      // t entries below K.  Only those can newly stand before the claim: the positions before pos0
                      // failed in this step's scan (re-tested when one passed the quick test and failed claim_full,
                      // stepFF), the blocks crossed earlier were tested at their crossing.
                      int pos0 = jj, p = jj;
                      while (U(left > 0)) {
                        if (!srt) {
                          int hint = 0;
                          if (nclaims >= 50) (void)S.w_choose_pivot_moved(nclaims, pos0, p, K, hint);
                          if (hint == 1) {
                            const int t = S.run_count_below(p, nclaims, K);
                            int fq = -1;
                            for (int base = 0; stepFF && base < pos0 && fq < 0; base += kWave) {
                              const int j = base + lane();
                              const uint64_t mq = wballot(j < pos0 && S.claim_quick(j, s, sflags, toltpl, pod));
                              if (mq) fq = base + ctz64(mq);
                            }
                            for (int base = p + 1; base <= p + t && fq < 0; base += kWave) {
                              const int j = base + lane();
                              const uint64_t mq = wballot(j <= p + t && S.claim_quick(j, s, sflags, toltpl, pod));
                              if (mq) fq = base + ctz64(mq);
                            }
                            sortsClosed++;
                            crossClosed++;
                            slow++;
                            srt = true;
                            const int64_t sb = (int64_t)(t + 1) * (8 + 16 * R);  // sort_claims' regather term
                            p += t;
                            if (UI(fq) >= 0) {
                              runMoves++;
                              S.run_materialise(pos0, p, K);
                              pos0 = p;
                              crossStops++;
                              stopC = c;
                              pendSortB = sb;  // the next pod's step: it meets the array sorted
                              break;
                            }
                            cross++;
                            sorts++;  // (the add() this pod would have entered)
                            per = span0 + sb + (int64_t)min((p / kWave + 1) * kWave, nclaims) * qbytes;
                          } else {
                            // the general re-sort: on the array as it stands, then as without KS_RUN_FUSE
                            runMoves += p != pos0;
                            S.run_materialise(pos0, p, K);
                            PH_BEGIN(tx);
                            int npos;
                            const int how = S.sort_claims(nclaims, p, npos);
                            exact += how == S.SORT_EXACT;
                            sortsClosed += how == S.SORT_CLOSED_FORM;
                            crossClosed += how == S.SORT_CLOSED_FORM;
                            slow++;
                            srt = true;
#ifdef KS_PHASE_STATS
                            {
                              const uint64_t dt = __builtin_amdgcn_s_memtime() - tx;
                              cyc[2] += dt;
                              cyc[5] -= dt;
                              S.xcyc[SS_CROSS] -= dt;
                            }
#endif
                            const int64_t sb = S.algbytes - ab0;
                            S.algbytes = ab0;
                            int fq = -1, np = UI(npos);
                            if (np >= 0) {
                              for (int base = 0; base < np && fq < 0; base += kWave) {
                                const int j = base + lane();
                                const uint64_t mq = wballot(j < np && S.claim_quick(j, s, sflags, toltpl, pod));
                                if (mq) fq = base + ctz64(mq);
                              }
                            } else {
                              for (int base = 0; base < nclaims; base += kWave) {
                                const int j = base + lane();
                                const uint64_t mq = wballot(j < nclaims && S.claim_quick(j, s, sflags, toltpl, pod));
                                const uint64_t mc = wballot(j < nclaims && S.s_order[j] == c);
                                if (fq < 0 && mq) fq = base + ctz64(mq);
                                if (mc) {
                                  np = base + ctz64(mc);
                                  break;
                                }
                              }
                              np = UI(np);
                            }
                            if (np < 0) {  // unreachable: s_order is a permutation of the claims
                              err = KE_STACK;
                              qlen = 0;
                              break;
                            }
                            pos0 = p = np;
                            fq = UI(fq);
                            if (fq >= 0 && fq < p) {
                              crossStops++;
                              stopC = c;
                              pendSortB = sb;
                              break;
                            }
                            cross++;
                            sorts++;
                            per = span0 + sb + (int64_t)min((p / kWave + 1) * kWave, nclaims) * qbytes;
                          }
                        }
                        const int nx = p + 1 < nclaims ? uni(S.s_okey[p + 1]) : 0x3fffffff;
                        int seg = nx - K + 1;
                        seg = seg < left ? seg : left;
                        if (seg <= 0) break;  // unreachable: the array is sorted here, so K <= nx
                        K += seg;
                        left -= seg;
                        k += seg;
                        credit += (int64_t)seg * per;
                        srt = K <= nx;
                      }
                      runMoves += p != pos0;
                      S.run_materialise(pos0, p, K);
                      pos = p;
                    } else
                    while (U(left > 0)) {
                      if (!srt) {
                        PH_BEGIN(tx);
                        int npos;  // the descent is the count just stored at `pos`
                        const int how = S.sort_claims(nclaims, SORTC ? pos : -1, npos);
                        exact += how == S.SORT_EXACT;
                        sortsClosed += how == S.SORT_CLOSED_FORM;
                        crossClosed += how == S.SORT_CLOSED_FORM;
                        runMoves++;
                        slow++;
                        srt = true;
#ifdef KS_PHASE_STATS
                        {  // the re-sort's cycles go to the sort phase, not to the commit phase around it
                          const uint64_t dt = __builtin_amdgcn_s_memtime() - tx;
                          cyc[2] += dt;
                          cyc[5] -= dt;
                          S.xcyc[SS_CROSS] -= dt;
                        }
#endif
                        const int64_t sb = S.algbytes - ab0;
                        S.algbytes = ab0;
                        // the first position passing the quick test; the claim's position: the closed form
                        // knows it, any other sort leaves it to be looked up in s_order
                        int fq = -1, np = UI(npos);
                        PH_BEGIN(tcq);
                        if (SORTC && np >= 0) {
                          // KS_CROSS_QUICK_FROM: the positions before the claim's old one hold claims this step did
                          // not touch, and the same pod failed the quick test on each of them (this step's scan, or
                          // an earlier crossing's re-test) -- unless one passed it and failed claim_full, whose
                          // recompute_max rewrote its headroom (stepFF).  Only the entries lifted over can newly
                          // stand before the claim: [old pos, new pos)
                          const int q0 = KS_CROSS_QUICK_FROM && LEAN && stepFF == 0 ? pos : 0;
                          for (int base = q0; base < np && fq < 0; base += kWave) {
                            const int j = base + lane();
                            const uint64_t mq = wballot(j < np && S.claim_quick(j, s, sflags, toltpl, pod));
                            if (mq) fq = base + ctz64(mq);
                          }
                        } else {
                          for (int base = 0; base < nclaims; base += kWave) {
                            const int j = base + lane();
                            const uint64_t mq = wballot(j < nclaims && S.claim_quick(j, s, sflags, toltpl, pod));
                            const uint64_t mc = wballot(j < nclaims && S.s_order[j] == c);
                            if (fq < 0 && mq) fq = base + ctz64(mq);
                            if (mc) {
                              np = base + ctz64(mc);
                              break;
                            }
                          }
                          np = UI(np);
                        }
                        SZPH_END(S, tcq, ZS_CROSS_QUICK);
                        if (np < 0) {  // unreachable: s_order is a permutation of the claims
                          err = KE_STACK;
                          qlen = 0;
                          break;
                        }
                        pos = np;
                        fq = UI(fq);
                        if (fq >= 0 && fq < pos) {
                          crossStops++;
                          stopC = c;
                          pendSortB = sb;  // the next pod's step: it meets the array sorted
                          break;
                        }
                        cross++;
                        sorts++;  // (the add() this pod would have entered)
                        per = span0 + sb + (int64_t)min((pos / kWave + 1) * kWave, nclaims) * qbytes;
                      }
                      const int nx = pos + 1 < nclaims ? uni(S.s_okey[pos + 1]) : 0x3fffffff;
                      int seg = nx - K + 1;
                      seg = seg < left ? seg : left;
                      if (seg <= 0) break;  // unreachable: the array is sorted here, so K <= nx
                      K += seg;
                      left -= seg;
                      k += seg;
                      credit += (int64_t)seg * per;
                      srt = K <= nx;
                      S.s_okey[pos] = K;  // wave-wide store of a uniform value
                      wsync();
                    }
                    SXPH_END(S, tcl, SS_CROSS);
                  } else {
                    const int cj = uni(S.s_okey[jj]);
                    const int nx = jj + 1 < nclaims ? uni(S.s_okey[jj + 1]) : 0x3fffffff;
                    const int M = m < nx - cj + 1 ? m : nx - cj + 1;
                    k = 0;
                    if (CAPB && S.capOver) {
                      S.capBoundSkips++;
                    } else {
                      k = inl ? S.template claim_run_cap<true>(c, pod, M) : S.template claim_run_cap<false>(c, pod, M);
#ifdef KS_PHASE_STATS
                      S.kcyc[KD_CAP_ZERO] += k == 0;
#endif
                    }
                    credit = (int64_t)k * (ab0 - abPop);  // each pod scanned as the first one did
                  }
                  if (k > 0) {
                    int64_t podk[RM];
#pragma unroll
                    for (int r = 0; r < RM; r++) podk[r] = (int64_t)k * pod[r];
                    int kcnt = 0;
                    PH_BEGIN(tbk);
                    if (inl) (void)S.template claim_full<true>(c, s, sflags, podk, req, nthr, kcnt);
                    else (void)S.template claim_full<false>(c, s, sflags, podk, req, nthr, kcnt);
                    // (KS_RUN_CROSS: the segments stored the count; the headroom at the final position is the
                    // regathered max - requests of the first pod's commit, less the run's requests)
                    const int kk = KS_RUN_CROSS ? 0 : k;
                    srt = inl ? S.template commit_bulk<true>(c, pos, nclaims, kk, podk, req, nthr, kcnt)
                              : S.template commit_bulk<false>(c, pos, nclaims, kk, podk, req, nthr, kcnt);
                    if constexpr (SORTC) dpos = srt ? -1 : pos;
                    S.algbytes = ab0 + credit;
                    SXPH_END(S, tbk, SS_BULK);
                    PH_BEGIN(tlg);
                    if (wi + k <= wn) {  // the run's pods are the window's next lanes
                      const int src = wi + lane() < kWave ? wi + lane() : kWave - 1;
                      S.log_batch(k, __shfl(w.p, src), c, nlog);
                    } else if constexpr (Solver<RT, TL, SIM, TOPO, LEAN, SLOG>::LOG_RUNS) {
                      // past the window: nothing was pushed back yet (only an ident run reaches here), so the run's
                      // pods are NewQueue's order from qhead on and one record describes its entries
                      S.log_run_record(k, qhead, c, nlog);
                      SYPH_END(S, tlg, YS_LOG_STORE);
                    } else if constexpr (KS_LOG_AHEAD) {
                      // past the window: the queue holds them (nothing pushed back yet).  Up to four 64-pod chunks
                      // are loaded before the first is stored: a load waits for the stores issued before it as well
                      // (vmcnt counts both), so 64 per load is one HBM round trip per chunk.  Lanes at or past k
                      // read the run's last pod (an index of the run, inside [0, P)); log_batch takes the first n.
                      for (int b = 0; b < k; b += 4 * kWave) {
                        int pv[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                          const int e = b + u * kWave + lane();
                          int pos = qhead + (e < k ? e : k - 1);
                          pos = pos >= P ? pos - P : pos;
                          pv[u] = W.queue[pos];
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                          const int left = k - b - u * kWave;
                          if (left > 0) S.log_batch(left < kWave ? left : kWave, pv[u], c, nlog);
                        }
                      }
                    } else {  // (KS_LOG_AHEAD=0: 64 per load)
                      for (int b = 0; b < k; b += kWave) {
                        int pos = qhead + b + lane();
                        pos = pos >= P ? pos - P : pos;
                        PH_BEGIN(tyq);
                        const int pv = b + lane() < k ? W.queue[pos] : 0;
                        PH_WAIT_LOADS();
                        SYPH_END(S, tyq, YS_LOG_LOAD);
                        PH_BEGIN(tyb);
                        S.log_batch(k - b < kWave ? k - b : kWave, pv, c, nlog);
                        SYPH_END(S, tyb, YS_LOG_STORE);
                      }
                    }
                    SXPH_END(S, tlg, SS_LOG);
                    qhead += k;
                    if (qhead >= P) qhead -= P;
                    qlen -= k;
                    pops += k;
                    wi += k;
                    if (wi > wn) wi = wn;  // the run reached past the window: refill at the loop head
                    runs++;
                    runPods += k;
                    if constexpr (CHAINB) kRun = k;
#ifdef KS_PHASE_STATS
                    skind = KD_CYC_RUN;
#endif
                  }
                }
              }
            }
          } else {
            // the quick bound was stale: tighten it to the exact max over the current options
            fullFails++;
            stepFF++;
            const int t = inl ? S.tplv(uni(S.lc.tpl[c])) : uni(W.c_tpl[c]);
            if (inl) S.template recompute_max<true>(c, S.lc.rem + (int64_t)c * d.TW, t, jj);
            else S.template recompute_max<false>(c, S.gc.rem + (int64_t)c * d.TW, t, jj);
          }
          PH_END(t5, 5);
        }
      }
    }
    // 3) new NodeClaim per template
    if (!U(placed)) {
      PH_BEGIN(t6);
      const int r = U(simNoClaim) ? S.sim_template_calls(hostCtr)
                                  : UI(S.try_templates(p, s, sflags, toltpl, pod, nclaims, nlog, hostCtr, srt));
      PH_END(t6, 6);
      nclaims = UI(nclaims);
      hostCtr = UI(hostCtr);
      srt = U(srt);
      dpos = -1;  // a descent left here is an appended claim's
      dapp = !srt;
      if (r < 0) {
        err = KE_CLAIM_CAP;
        if constexpr (decltype(S)::TPL_TABLE_CHECK) err = r == -2 ? KE_TPL_TABLE : KE_CLAIM_CAP;
        break;
      }
      if (r == 1) placed = true;
      if constexpr (CHAINB) onClaim = r == 1;
#ifdef KS_PHASE_STATS
      if (r == 1) skind = KD_CYC_OPEN;
#endif
      if (r == 2) {  // no templates: add() returns a nil error
        W.pod_status[p] = ST_SCHEDULED;  // wave-wide store of a uniform value
        placed = true;
      }
    }
    if (U(placed)) {
      if constexpr (CHAINB) {
        // Is the next queue pod of this pod's identical-pod run?  The claim runs' identity: while nothing was pushed
        // back, the popped pod's run length less the pods placed since; otherwise the window's next lane with the same
        // template tolerations, tolerations and requests, not stale.  (A window that ended: the next pod takes a
        // whole step.)
        if (onClaim && qlen > 0) {
          bool nx = false;
          if (ident) {
            nx = rlp - 1 - kRun > 0;
          } else if (wi < wn) {
            bool same = lane() == wi && w.toltpl == toltpl && w.tol0 == tol0 && w.tol1 == tol1;
#pragma unroll
            for (int r = 0; r < RM; r++) {
              if (RT == 0 && r >= R) break;
              same &= w.req[r] == pod[r];
            }
            same &= !((uint32_t)(w.ll >> 32) == epoch && (uint32_t)w.ll == (uint32_t)qlen);
            nx = wballot(same) != 0;
          }
          chain = nx;
        }
      }
#ifdef KS_PHASE_STATS
      S.kcyc[skind] += __builtin_amdgcn_s_memtime() - t0;
      S.kcyc[skind + KD_N_OPEN] += 1;
#endif
      // SIM: the epilogue reads the final status; only a pod that failed before needs a store
      if (SIM && rdl(w.st, wi - 1) == ST_FAILED) W.pod_status[p] = ST_SCHEDULED;  // (wave-wide, uniform)
      continue;
    }
    // failure: Preferences.Relax (preferences.go:38) + Queue.Push (queue.go:64-71)
    if constexpr (LEAN && !SIM) {
      // pods sharing a UID share Queue.Pop's staleness entry, which the LEAN pop does not re-read: a Solve
      // with shared UIDs leaves here, before its first push-back, and the host re-runs it non-LEAN
      if (d.dupUids) {
        err = KE_LEAN_EXIT;
        break;
      }
    }
    if (SIM && ident) S.sim_queue_init(P);  // the simulation's first push-back: its queue state, lazily
    const int s0 = D.pod_state0[g], ns = D.pod_nstate[g];
    const bool relaxed = U(s - s0 + 1 < ns);
    W.pod_status[p] = ST_FAILED;  // wave-wide stores of uniform values
    W.pod_fstate[p] = s;
    if (relaxed) W.pod_state[p] = s + 1;
    if (relaxed) epoch++;
    anyRelaxed = anyRelaxed || relaxed;
    if (TOPO && relaxed) S.topo_activate_state(s + 1, nclaims, hostCtr);  // Topology.Update (scheduler.go:160-170)
    int tail = qhead + qlen;
    if (tail >= P) tail -= P;
    W.queue[tail] = p;  // wave-wide store of a uniform value
    qlen++;
    pushed = true;
    ident = false;
    if (!relaxed) W.last_len[uid] = ((uint64_t)epoch << 32) | (uint32_t)qlen;  // (wave-wide, uniform)
  }
  if constexpr (MWK) {  // the helpers' contributions, then they leave
    mw_post(MW_EXIT, 0, pod, 0, 0, 0);
    mw_barrier();  // B2
    bool hall = true;
    int64_t hab = 0;
#pragma unroll
    for (int q = 1; q < kMwWaves; q++) {
      hall = hall && mb[MB_ALL + q] != 0;
      hab += (int64_t)mb_ld64(mb, MB_AB + 2 * q);
    }
    allSched = allSched && ub(hall);
    S.algbytes += uni64(hab);
  }
  S.log_flush(nlog);
  // write back LDS-resident claim state for the host
  for (int i = lane(); i < nclaims; i += kWave) W.order[i] = S.s_order[i];
  if constexpr (SLOG) {  // len(Pods) per claim id, for the host's check of the log (the workspace holds max(P, 1) claims)
    for (int i = lane(); i < nclaims; i += kWave) {
      const int c = S.s_order[i];
      if (c >= 0 && c < (P > 1 ? P : 1)) W.c_npods[c] = S.s_okey[i];
    }
  }
  const int kl = nclaims < pl.KL ? nclaims : pl.KL;
  for (int i = lane(); i < kl * R; i += kWave) W.c_req[i] = S.lc.req[i];
  for (int i = lane(); i < kl * d.TW; i += kWave) W.c_rem[i] = S.lc.rem[i];
  if (lane() == 0) {
    W.counters[CT_NCLAIMS] = nclaims;
    W.counters[CT_NLOG] = nlog;
    W.counters[CT_HOSTCTR] = hostCtr;
    W.counters[CT_ERROR] = err;
    W.counters[CT_POPS] = pops;
    W.counters[CT_ALGBYTES] = S.algbytes;
    W.counters[CT_SORTS] = sorts;
    W.counters[CT_SORT_SLOW] = slow;
    W.counters[CT_CLAIM_FULL] = fulls;
    W.counters[CT_CLAIM_QUICK_FAIL] = fullFails;
    W.counters[CT_WINDOWS] = windows;
    W.counters[CT_RUNS] = runs;
    W.counters[CT_RUN_PODS] = runPods;
    W.counters[CT_SORT_EXACT] = exact;
    W.counters[CT_RUN_CROSS] = cross;
    W.counters[CT_RUN_CROSS_STOPS] = crossStops;
    W.counters[CT_RUN_CROSS_LOST] = crossLost;
    W.counters[CT_SORT_CLOSED] = sortsClosed;
    W.counters[CT_TPL_MEMO_HITS] = S.memoHits;
    W.counters[CT_RUN_CAP_FRONT] = S.capFront;
    W.counters[CT_RUN_CAP_FULL] = S.capFull;
    W.counters[CT_RUN_CROSS_CLOSED] = crossClosed;
    W.counters[CT_RUN_MOVES] = runMoves;
    W.counters[CT_TPL_MASK_FILLS] = S.maskFills;
    W.counters[CT_TPL_MASK_HITS] = S.maskHits;
    W.counters[CT_RUN_RECS] = S.runRecs;
    if constexpr (decltype(S)::TPL_TABLE) W.counters[CT_TPL_TABLE_HITS] = S.tableHits.n;
    if constexpr (decltype(S)::SORT_REGS) {  // (k_init zeroed them: the other instantiations' code stays as it was)
      W.counters[CT_SORT_REGS] = S.sortsRegs;
      W.counters[CT_SORT_REGS_BAIL] = S.sortRegsBail;
      W.counters[CT_SORT_REGS_OVER] = S.sortRegsOver;
    }
    if constexpr (decltype(S)::RESORT_CTR) {  // (k_init zeroed them: the other instantiations' code stays as it was)
      W.counters[CT_SORT_CROSS50] = S.rsc.cross50;
      W.counters[CT_PIVOT_ARITH] = S.rsc.arith;
      W.counters[CT_SORT_APPEND50] = S.rsc.append50;
      W.counters[CT_APPEND_CLOSED] = S.rsc.appClosed;
      W.counters[CT_PIVOT_ARITH_DIFF] = S.rsc.diff;
    }
    if constexpr (CAPB) W.counters[CT_CAP_BOUND_SKIPS] = S.capBoundSkips;
    if constexpr (CHAINB) W.counters[CT_CHAIN_PODS] = chainPods;
    if constexpr (decltype(S)::THR_BATCH) {
      W.counters[CT_THR_BATCH_CALLS] = S.thrBatchCalls;
      W.counters[CT_THR_MULTI_CHUNK] = S.thrMultiChunk;
    }
#ifdef KS_PHASE_STATS
    for (int i = 0; i < 7; i++) W.counters[CT_CYC_POP + i] = (int64_t)cyc[i];
    W.counters[CT_CYC_TOTAL] = (int64_t)(__builtin_amdgcn_s_memtime() - tstart);
    W.counters[CT_CYC_NCOMMIT] = (int64_t)cyc[7];
    for (int i = 0; i < 4; i++) W.counters[CT_CYC_SUB + i] = (int64_t)S.scyc[i];
    for (int i = 0; i < 8; i++) W.counters[CT_FINE + i] = (int64_t)fcyc[i];
    for (int i = 0; i < 12; i++) W.counters[CT_STEP + i] = (int64_t)S.xcyc[i];
    for (int i = 0; i < 3; i++) W.counters[CT_CYC_EXACT_BY_N + i] = (int64_t)S.ecyc[i];
    W.counters[CT_CLOSED_SHIFT_DIFF] = S.shiftDiff;
    for (int i = 0; i < 6; i++) W.counters[CT_CYC_SPLIT + i] = (int64_t)S.ycyc[i];
    for (int i = 0; i < 9; i++) W.counters[CT_KIND + i] = (int64_t)S.kcyc[i];
    for (int i = 0; i < 3; i++) W.counters[CT_CYC_RESORT + i] = (int64_t)S.zcyc[i];
    W.counters[CT_CYC_RESORT + ZS_PIVOT] += (int64_t)S.pivcyc;  // the samples taken inside closed_crossing
#endif
  }
  if constexpr (SIM) S.sim_record(P, nclaims, hostCtr, allSched, err, !ident, anyRelaxed);
