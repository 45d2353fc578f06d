/* karpenter_amd.h — C-ABI of the MI355X Karpenter scheduler hot path (libkarpenter_amd.so).
 *
 * Drop-in boundary for pkg/controllers/provisioning/scheduling in the reference
 * (/root/reference, paths relative to it).  A Go cgo shim marshals the arguments of
 *   NewScheduler(ctx, kubeClient, nodeClaimTemplates, nodePools, cluster, stateNodes, topology,
 *                instanceTypes, daemonSetPods, recorder, opts)        scheduler.go:49-83
 * plus the `pods` argument of
 *   (*Scheduler).Solve(ctx, pods) *Results                             scheduler.go:140-189
 * into one JSON snapshot (see INTEGRATION.md for the schema and the shim), and rebuilds
 *   Results{NewNodeClaims, ExistingNodes, PodErrors}                  scheduler.go:102-106
 * from the result, mapping pod indices back to the caller's *v1.Pod pointers.
 *
 * Plain C types only; no torch or HIP types cross this boundary.  Every call returns 0 on success
 * or a negative KS_ERR_* code; ks_last_error() then holds thread-local text.  A ks_problem is not
 * re-entrant (mirrors the single-goroutine Scheduler); use one per thread.
 */
#ifndef KARPENTER_AMD_H_
#define KARPENTER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_OK 0
#define KS_ERR_PARSE -1       /* malformed snapshot JSON / quantity */
#define KS_ERR_UNSUPPORTED -2 /* input uses a feature this build does not encode (message says which) */
#define KS_ERR_CAPACITY -3    /* encoding limits exceeded (keys > 64, taints > 128, claims > cap) */
#define KS_ERR_HIP -4         /* HIP runtime error (no device, launch failure, fault) */
#define KS_ERR_INTERNAL -5    /* kernel reported an inconsistent state (iteration cap, overflow) */
#define KS_ERR_ARG -6

typedef struct ks_problem ks_problem;
typedef struct ks_results ks_results;

typedef struct ks_solve_opts {
  int device;          /* HIP device ordinal; -1 = current device */
  int simulation_mode; /* SchedulerOptions.SimulationMode (scheduler.go:44-47); decisions identical */
  int replicas;        /* >1: solve `replicas` independent copies in one launch (one wavefront each) */
  int timing_only;     /* 1: do not copy results back (counters and timings only); benchmarks */
  int lds_budget;      /* bytes of LDS per Solve; 0 = automatic (tests use small budgets to force the
                          HBM-resident claim path) */
  int launch_lists;    /* 1: also compute every NewNodeClaim's launch list on the device
                          (ks_results_nodeclaim_launch); 0: no launch data, Results as without the field.
                          Ignored with timing_only.  ks_cons_run / ks_cons_disrupt: also compute the
                          launch list of every replacement (ks_cons_claim_launch,
                          ks_cons_disrupt_launch); 0: nothing is computed and every document is as
                          without the field */
  int reserved[2];
} ks_solve_opts;

/* NewScheduler equivalent: parse + encode the snapshot and upload it to HBM.  Replaces the Go
 * allocation-heavy construction at scheduler.go:49-83 + nodeclaimtemplate.go:43-53 +
 * existingnode.go:40-62; the caller keeps ownership of `snapshot_json`. */
int ks_problem_create(const char* snapshot_json, size_t len, ks_problem** out);
void ks_problem_free(ks_problem* p);

/* Binary snapshot of an encoded problem (the whole host model NewScheduler built: universes, tables, pods,
 * relaxation chains, topology): ks_problem_save writes it (free with ks_free); ks_problem_create_binary
 * rebuilds the problem from it and uploads it, skipping the JSON parse and the encode.  A snapshot is tied to
 * the library build that wrote it (a blob from another build is refused with KS_ERR_PARSE). */
int ks_problem_save(const ks_problem* p, void** buf, size_t* len);
int ks_problem_create_binary(const void* buf, size_t len, ks_problem** out);
/* Host-only (no device): encode snapshot_json, save it, load the bytes and save again; KS_OK when the two
 * byte strings are identical.  *bytes: the snapshot size. */
int ks_snapshot_check(const char* snapshot_json, size_t len, size_t* bytes);
/* Host-only (no device): the binary snapshot of snapshot_json, as ks_problem_save would write it for a
 * problem created from that JSON (free with ks_free), e.g. to convert fixtures offline. */
int ks_problem_encode_binary(const char* snapshot_json, size_t len, void** buf, size_t* blen);
/* Host-only (no device): the load-time checks of ks_problem_create_binary (header, lengths backed by bytes,
 * offset tables, every table against the dims and every stored index against its table): KS_OK, or
 * KS_ERR_PARSE for a truncated, foreign or internally inconsistent blob. */
int ks_problem_check_binary(const void* buf, size_t len);

/* Host-only encode of a snapshot (no device needed): returns JSON with the universe sizes (keys,
 * value words, resources "R", instance types, relaxation states), "lean" / "negReq" (resource-only pods /
 * some negative request), "plans" (the LDS plan at the default and a few reduced budgets), "widePlans" (per budget of "plans", the two
 * plans ks_solve re-plans to when a Solve outgrows the plan's NodeClaim capacity "KO"), "FNR" (relaxation
 * states with label requirements: the rows of k_feasibility_nodes), "keyValues" (per key of "keyNames", the
 * size of its value universe) and "coveredKeys" (the keys k_feasibility's rows decide).  Topology: "tgCntWords"
 * (count words), "tgSmall" (the prefix of small-key groups), "TK" and "topologyKeys" (the distinct topology keys in
 * key-slot order), "topologyGroups" ([key slot, domains, in the small prefix, type, hostname] per group); each plan
 * has "tcl" / "tdl" (count words / node-domain words it keeps in LDS).
 * Launch lists: "nameRank" (per template, for each position of its instance-type list, the rank of the instance
 * type's name in bytewise string order among all instance types: OrderByPrice's tie-break as the device reads it)
 * and "launchListsRefusal" ("" or the message a Solve with launch_lists set fails with: a template listing two
 * instance types of one name).
 * Diagnostics / CPU tests. */
int ks_problem_inspect(const char* snapshot_json, size_t len, char** dims_json);
/* The same document for a binary snapshot (what ks_problem_create_binary would load), no device. */
int ks_problem_inspect_binary(const void* buf, size_t len, char** dims_json);

/* Test and diagnostic entry: read back one of the two static feasibility tables a Solve computes before
 * k_solve.  which = 0: k_feasibility's pod-state x instance-type rows; which = 1: k_feasibility_nodes's
 * pod-state x existing-node rows.  The call makes the launch a Solve makes, on the problem's stream, over
 * the table filled with 0xA5 bytes (a word the kernel does not store reads back as 0xA5A5A5A5), waits for
 * it and copies the table out; a later Solve rewrites the table as usual.  KS_ERR_UNSUPPORTED when the
 * table is off for this problem (no pod label requirements, no existing nodes, KS_NO_FEASIBILITY /
 * KS_NO_NODE_ROWS).
 *   words (free with ks_free), n_words: which = 0: S * NTPL rows of TW words, row s * NTPL + t; bit p of a row
 *     is position p of template t's instance-type list.  which = 1: FNR rows of ceil(N / 32) words, row
 *     stateNodeRow[s]; bit n is existing node n in device order.
 *   meta_json (free with ks_free): {"S", "NTPL", "TW", "N", "FNR", "podState0": [per pod, its first relaxation
 *     state], "podNState": [per pod, the length of its chain], "stateNodeRow": [per state, its node row or -1],
 *     "stateTolTpl": [per state, the bitmask of the templates whose taints it tolerates], "templates":
 *     [{"instanceTypes": [names in position order], "irregular": [TW words: the positions whose instance
 *     type holds a complement requirement]}], "nodes": [existing-node names in device order], "coveredKeys":
 *     [the label keys the instance-type rows decide: those no instance type holds with more than one value]}. */
int ks_problem_feasibility_rows(ks_problem* p, int which, char** meta_json, uint32_t** words, size_t* n_words);

/* The static feasibility matrix: every relaxation state of every pod against every NodeClaimTemplate's instance
 * types and every existing node, from the problem's static tables alone (no Solve).
 *
 * Template row (s, t): what Scheduler.add's template phase gives a fresh NodeClaim of template t for the pod of
 * state s before any commit, tested in this order: the NodePool's remaining limits (FC_LIMITS), the template's
 * taints (FC_TAINTS), Compatible + Add of the requirements (FC_COMPAT), then per instance type Intersects, Fits
 * with the template's daemon overhead and an available offering (FC_NO_IT | filterResults flags << 8).  code is
 * 0 when the row has options; count is their number; the TW words are the options as template positions (all
 * zero in a failing row and past the template's list).
 * Node row s: bit n is set iff existing node n accepts the pod on its initial state: taints tolerated, no host
 * port conflict, Fits(node requests + pod, available), strict Compatible of the labels.  ceil(N / 32) words,
 * bits past N zero; count is the number of set bits.
 *
 * Topology and volume limits are not evaluated ("ignores" in the meta document; it lists the states that own
 * topology groups and carries "volAny"): for those the rows are an upper bound.  Within a Solve requests and
 * host ports only grow, requirements only narrow and remaining limits only shrink, so a clear bit holds for
 * every Solve of the problem; a set bit is exact for an empty scheduler without topology.  A problem with a
 * negative request is refused with KS_ERR_UNSUPPORTED (Fits is not monotone then).
 *
 * where = 0: two kernels on the device the problem lives on (opts->device as for ks_solve; opts may be NULL),
 * on the problem's stream; where = 1: the same definitions in plain loops on the host, no device call.
 * ks_problem_create_host builds a problem without a device for where = 1 (ks_solve on it fails with KS_ERR_HIP).
 *
 * ks_feasibility_meta (free with ks_free): {"S", "NTPL", "N", "TW", "NWN", "podState0", "podNState", "statePod",
 * "templates": [{"nodePool", "instanceTypes": [names in position order]}], "nodes": [names in device order],
 * "ignores": ["topology", "volumeLimits"], "topologyStates": [states that own a topology group], "volAny",
 * "codes": {"FC_NONE", "FC_LIMITS", "FC_TAINTS", "FC_COMPAT", "FC_NO_IT", "FF_REQ", "FF_FITS", "FF_OFF",
 * "FF_REQ_FITS", "FF_REQ_OFF", "FF_FITS_OFF"}}.
 * The row accessors return pointers into the handle (valid until ks_feasibility_free); KS_ERR_ARG for a state or
 * template out of range.  ks_feasibility_timing: where = 0: the two kernels' time by events, the table bytes
 * they address and the bytes of the rows they write; where = 1: kernel_ms 0 and the same byte counts. */
typedef struct ks_feasibility ks_feasibility;
int ks_problem_create_host(const char* snapshot_json, size_t len, ks_problem** out);
int ks_problem_static_feasibility(ks_problem* p, const ks_solve_opts* opts, int where, ks_feasibility** out);
void ks_feasibility_free(ks_feasibility* f);
int ks_feasibility_meta(const ks_feasibility* f, char** meta_json);
int ks_feasibility_template_row(const ks_feasibility* f, int state, int tpl, uint32_t* code, int32_t* count,
                                const uint32_t** words, int* n_words);
int ks_feasibility_node_row(const ks_feasibility* f, int state, int32_t* count, const uint32_t** words, int* n_words);
int ks_feasibility_timing(const ks_feasibility* f, double* kernel_ms, int64_t* bytes_read, int64_t* bytes_written);
/* Bulk view of the five arrays (what the Python mirror copies): tpl_code [S][NTPL], tpl_count [S][NTPL],
 * tpl_options [S][NTPL][TW], node_bits [S][NWN], node_count [S]; dims: S, NTPL, N, TW, NWN.  Any pointer may be
 * NULL. */
int ks_feasibility_arrays(const ks_feasibility* f, int dims[5], const uint32_t** tpl_code, const int32_t** tpl_count,
                          const uint32_t** tpl_options, const uint32_t** node_bits, const int32_t** node_count);
/* The two kernels' times separately (where = 0; zeros for where = 1). */
int ks_feasibility_kernel_times(const ks_feasibility* f, double* templates_ms, double* nodes_ms);

/* Test and diagnostic entries: what the queue-preparation kernels (ks_queue.hip) read and write.  None of them
 * runs k_solve.
 *
 * ks_problem_queue_inputs: host-only (no device).  The encoded inputs of NewQueue's sort and of the identical-pod
 * run lengths, so a reference never reads what a kernel wrote.  JSON {"P", "R", "resources": [names in column
 * order], "resShift": [per resource, the decimal shift of its device unit: 10^shift nano-units], "uids": [per pod], "sortKeys": [per pod, the four components -cpu, -memory, creation second, uid rank
 * (queue.go:83-112)], "skMin": [4], "skBits": [4], "lean", "dupUids", "hostOrder": null | [the pdqsort-emulated
 * order the device reads when pods tie on the whole key], "podReq": [per pod, R int64], "podS0": [per pod, the four
 * words of its first relaxation state: toleration mask low / high, template-toleration set, state flags],
 * "podFlags": [per pod], "PF_PROVISIONABLE": the provisionable bit of podFlags}.  Free with ks_free. */
int ks_problem_queue_inputs(const char* snapshot_json, size_t len, char** out_json);
/* The queue launches a Solve makes before k_solve, on the problem's stream, into buffers of this call filled with
 * 0xA5 bytes first (a word no kernel stores reads back as 0xA5A5A5A5): the NewQueue radix-sort chain, or the
 * uploaded host order when pods tie (*device_sorted 0), then -- for a lean problem -- the strict identical-pod run
 * lengths over that order.  order: P int32 pod indices; run_len: P int32, NULL when the problem is not lean.
 * Free both with ks_free. */
int ks_problem_queue_readback(ks_problem* p, int32_t** order, int32_t** run_len, size_t* n, int* device_sorted);
/* The re-sort of s.newNodeClaims (scheduler.go:247) as the Solve kernel does it, on arrays of the caller's choosing:
 * no problem, no Solve.  keys / order: n <= 1024 pod counts and claim ids 0 .. n - 1 per sorted position, sorted in
 * place.  claim_tpl [n] / claim_head [n][R] (R 3 or 4) are per-claim values from which the kernel fills its two other
 * position arrays before the sort; ptpl [n] / phead [n][R] receive those arrays as the sort leaves them (equal to
 * claim_tpl / claim_head of order[j] at every position j).  mode 0: the general path (a claim was appended);
 * mode 1: the path after a count increment at pos -- keys non-decreasing but for keys[pos] > keys[pos + 1] at most
 * -- which takes the closed form where the kernel does.  *how (may be NULL): 0 partialInsertionSort finished it,
 * 1 the exact pdqsort ran, 2 the closed form.  device < 0: the same call computes the expected value on the host
 * with Go's pdqsort_func (*how 1). */
int ks_claim_sort_probe(int device, int mode, int pos, int n, int R, int32_t* keys, int32_t* order,
                        const int32_t* claim_tpl, const int64_t* claim_head, int32_t* ptpl, int64_t* phead, int* how);
/* The same with the path the general re-sort took in *path (may be NULL): 0 none (the closed form, or a build
 * without the register copy), 1 it finished on the copy held in registers (up to 64 entries as shipped, 128 in a
 * -DKS_SORT_REGS_N64=0 build), 2 the copy was abandoned on a failed invariant, 3 the array has more entries than the
 * copy holds (2 and 3: the LDS code sorted it).  device -3: the host's lane model of the 64-entry copy in place of
 * Go's pdqsort_func (-2: of the 128-entry form); *path then also holds its breakPatterns calls << 8 and its heapSort
 * calls << 20. */
int ks_claim_sort_probe_path(int device, int mode, int pos, int n, int R, int32_t* keys, int32_t* order,
                             const int32_t* claim_tpl, const int64_t* claim_head, int32_t* ptpl, int64_t* phead,
                             int* how, int* path);
/* The same for a claim appended behind greater counts -- keys non-decreasing on [0, n - 1), keys[n - 1] below
 * keys[n - 2] -- with that origin told to the kernel, as the Solve tells it: from 50 entries on the re-sort is then a
 * closed form (the new entry goes behind the last count not above its own, the entries after it move one place).
 * *how as above (0 when the closed form ran); *taken (may be NULL): 1 when it ran.  device < 0: Go's pdqsort_func on
 * the host (*how 1, *taken 0). */
int ks_claim_sort_probe_append(int device, int n, int R, int32_t* keys, int32_t* order, const int32_t* claim_tpl,
                               const int64_t* claim_head, int32_t* ptpl, int64_t* phead, int* how, int* taken);
/* k_rec_headers (the device-side record invariants and header compaction of a consolidation pass) without a
 * handle.  records: the passes' record batches back to back, pass i holding pass_ns[i] records of RF_HDR + 3 * TW
 * int32 words; tpl_beg: ntpl + 1 offsets, template t's instance-type list has tpl_beg[t + 1] - tpl_beg[t] <= 32 * TW
 * entries.  The status words and the block counter are allocated and initialised once, as a handle does it, and
 * every pass runs over them without re-initialisation.  headers: every pass's pass_ns[i] * RF_HDR words (buffers
 * filled with 0xA5 bytes before each pass); status: two published words per pass; verdicts_json: per pass, per
 * record, the message the host's check of the same record throws, "" when it passes (headers and status both NULL:
 * these verdicts alone, no device).  meta_json: {"RF_HDR",
 * "RF": {field: index}, "CA": {action: value}, "KE": {kernel error: value}};
 * n_passes 0 returns the metadata alone (no device needed).  Free the JSON with ks_free. */
int ks_rec_headers_run(const int32_t* records, const int32_t* pass_ns, int n_passes, int TW, const int32_t* tpl_beg,
                       int ntpl, int32_t* headers, uint64_t* status, char** verdicts_json, char** meta_json);

/* Solve (scheduler.go:140-189) on the GPU.  Fresh scheduler state every call (a Scheduler is
 * single-use in production, scheduler.go:49 is called per Schedule / per simulation). */
int ks_solve(ks_problem* p, const ks_solve_opts* opts, ks_results** out);
void ks_results_free(ks_results* r);

/* Results as canonical JSON: {"newNodeClaims":[{nodePoolName, hostname, pods[], instanceTypeOptions[],
 * requests{}, requirements[], requirementsString}], "existingNodes":[{name, pods[]}],
 * "podErrors":{"<pod index>": "<error text>"}, "stats":{<solve counters>, "route":{...}}}.
 * "stats"."route" names the k_solve instantiation the Solve launched: {"family": "solve" | "solve_topo",
 * "rt": 3 | 4 | 0 (the live-resource count the kernel is specialised for; 0: the generic code, any count),
 * "tl": 0 | 1 (instance-type tables LDS-resident), "lean": 0 | 1 (the resource-only instantiation),
 * "n": work items, "launches": [the same fields for every launch of this Solve, in order]}.  A Solve that
 * re-plans (a lean Solve leaving for the non-lean code, a wider NodeClaim plan) has one entry per launch;
 * the outer fields are the last launch's.  "stats"."plan" is that launch's LDS plan: {"wide": 0 | 1 | 2 (the
 * re-plan level for NodeClaim capacity), "KO" (NodeClaims per Solve), "KL" (of them LDS-resident), "talloc",
 * "lds" (bytes)}.  Free with ks_free. */
int ks_results_json(const ks_results* r, char** json_out);

/* Structured accessors for a cgo shim (no JSON on the hot return path). */
int ks_results_num_new_nodeclaims(const ks_results* r);
int ks_results_nodeclaim(const ks_results* r, int i, int* template_index, const int32_t** pods, int* n_pods,
                         const int32_t** instance_types, int* n_instance_types);
int ks_results_num_existing_nodes(const ks_results* r);
int ks_results_existing_node(const ks_results* r, int i, int* state_node_index, const int32_t** pods, int* n_pods);
int ks_results_num_pod_errors(const ks_results* r);
int ks_results_pod_error(const ks_results* r, int i, int* pod_index, const char** message);

/* One key of a NodeClaim's Requirements (pkg/scheduling/requirement.go:33-280), as a cgo shim rebuilds
 * it: Operator() ("In", "NotIn", "Exists", "DoesNotExist"; Gt/Lt read as "Exists" with bounds,
 * requirement.go:197-208), the value set in sorted order, and the Gt / Lt bounds. */
typedef struct ks_requirement {
  const char* key;
  const char* op;
  int n_values;
  const char* const* values;
  int has_gt, has_lt;
  int64_t gt, lt;
} ks_requirement;
/* NodeClaim i's Spec.Resources.Requests (nodeclaim.go:35-42, scheduler.go:102-106): resource names in
 * name order with canonical resource.Quantity.String() text.  Arrays live as long as r. */
int ks_results_nodeclaim_requests(const ks_results* r, int i, int* n, const char* const** names,
                                  const char* const** quantities);
/* NodeClaim i's Requirements after FinalizeScheduling (hostname removed, nodeclaim.go:123-128), one entry
 * per key in key order (what consolidation.go:134-188 reads from NewNodeClaims[0]). */
int ks_results_nodeclaim_requirements(const ks_results* r, int i, int* n, const ks_requirement** reqs);
/* NodeClaimTemplate.ToNodeClaim's launch list (nodeclaimtemplate.go:55-60) of NodeClaim i: its instance-type
 * options in InstanceTypes.OrderByPrice order (types.go:62-79), cut to the first 100.  An option's price is its
 * cheapest available offering that the NodeClaim's zone and capacity-type requirements allow (Offerings.Available()
 * .Requirements(reqs).Cheapest(), types.go:147-166; a key the requirements do not hold allows every value), and
 * math.MaxFloat64 when no offering is allowed (which the Solve's own offering filter rules out for a NodeClaim it
 * returns); equal prices (-0.0 equals 0.0) are ordered by name, bytewise.  Computed by a kernel after the Solve
 * when ks_solve_opts.launch_lists is set, from the claim state and the offering tables resident on the device,
 * and checked on the host before it is handed out.
 *   instance_types / prices: *n entries each (indices into the snapshot's instanceTypes; the price that ordered
 *   the entry), *n = min(*n_options, 100); *n_options: len(InstanceTypeOptions).  Arrays live as long as r; any
 *   out pointer may be NULL.
 * KS_ERR_ARG for i out of range and for a Results whose Solve did not set launch_lists.  A Solve with launch_lists
 * set fails with KS_ERR_UNSUPPORTED when a template lists two instance types of the same name (the order of equal
 * keys is then sort.Slice's, not a function of the keys), and with KS_ERR_CAPACITY when a template's list is too
 * long for the kernel's LDS (more than about 6000 instance types). */
int ks_results_nodeclaim_launch(const ks_results* r, int i, const int32_t** instance_types, const double** prices,
                                int* n, int* n_options);
/* HIP-event time of the launch-list kernel of this Solve (milliseconds); 0 when it did not run. */
double ks_results_launch_ms(const ks_results* r);

/* Device time of the solve kernel(s) of the last ks_solve, measured with HIP events on the
 * stream the kernel ran on (milliseconds). */
double ks_results_kernel_ms(const ks_results* r);
/* The k_solve launch alone (the dominant kernel; excludes workspace init and the queue sort). */
double ks_results_solve_kernel_ms(const ks_results* r);
/* k_feasibility (the static pod-state x instance-type rows) inside this Solve: HIP-event time and its
 * algorithmic bytes; 0 when the problem has no pod label requirements (the kernel is not launched). */
double ks_results_feasibility_ms(const ks_results* r);
double ks_results_feasibility_bytes(const ks_results* r);
/* k_feasibility_nodes (the static pod-state x existing-node rows: taints + strict Compatible,
 * existingnode.go:64-124) inside this Solve: HIP-event time and algorithmic bytes; 0 when not launched
 * (no pod label requirements or no existing nodes). */
double ks_results_node_feasibility_ms(const ks_results* r);
double ks_results_node_feasibility_bytes(const ks_results* r);
/* Algorithmic bytes the solve scanned (SURVEY.md §8d formula, counted by the kernel). */
double ks_results_algorithmic_bytes(const ks_results* r);

/* ---- Consolidation (pkg/controllers/disruption) ------------------------------------------------
 * ks_cons_create replaces the per-simulation NewScheduler calls of simulateScheduling
 * (helpers.go:73-127) for one disruption pass: the cluster snapshot (state nodes
 * with their pods, pending pods, candidate node names, NodePools, instance types) is encoded once.
 * Candidates are built and ordered like NewCandidate + sortAndFilterCandidates (types.go:54-113,
 * consolidation.go:73-83).  The simulations are every multi-node prefix firstNConsolidationOption
 * can probe (multinodeconsolidation.go:87-137) and one per candidate (singlenodeconsolidation.go:
 * 42-88); each ends in the computeConsolidation decision (consolidation.go:113-194) on the GPU. */
typedef struct ks_cons ks_cons;
int ks_cons_create(const char* snapshot_json, size_t len, ks_cons** out);
/* Binary snapshot of a consolidation handle (host model + candidates in disruption-cost order + the
 * simulation plan), as for ks_problem_save / ks_problem_create_binary. */
int ks_cons_save(const ks_cons* c, void** buf, size_t* len);
int ks_cons_create_binary(const void* buf, size_t len, ks_cons** out);
/* Host-only (no device): JSON {candidates:[{name, disruptionCost, pods}], sims, multiPrefixes, recordBytes,
 * R, G, lean, negReq, simPlan:{KO, KL, talloc, tsort, tcl, tdl, lds}} (simPlan: the LDS plan of a world-1 pass)
 * plus tgSmall, tgCntWords, TK, topologyKeys and topologyGroups as ks_problem_inspect reports them. */
int ks_cons_inspect(const char* snapshot_json, size_t len, char** out_json);
/* Cluster-state events between two passes against the resident handle (replaces re-reading the cluster
 * and rebuilding the scheduler per pass: state/cluster.go:220-512 UpdatePod/DeletePod/DeleteNode,
 * provisioner.go:204-296).  update_json: {"deletePods":[uid], "bindPods":[{"uid","node"}],
 * "removeNodes":[name]}, applied in that order: a deleted pod frees its node's requests; a bound pod
 * (pending until now) is Running on an active node and takes its requests; a removed node takes its pods
 * with it and returns its capacity to its NodePool's limits.  In a topology cluster the shared NewTopology
 * counts follow (topology.go:61-85,190-230; the snapshot's clusterPods lose deleted / removed-node pods and
 * gain bound ones).  Candidates, their costs and order, and the simulations are re-derived; the next
 * ks_cons_run sees the new state.  All or nothing: KS_ERR_ARG for unknown / already-deleted / not-pending
 * pods or unknown nodes.  KS_ERR_UNSUPPORTED (rebuild with ks_cons_create there) only for: deleting or binding a
 * pod that mounts volumes in a cluster with volume limits (pods without volumes and node removals are applied
 * there too); binding a pod with host ports (deleting one drops its node's entries); and binding a pod that
 * counts in a topology domain or inverse group the handle does not hold.  A topology group that only a
 * relaxation creates after the update becomes a late group in place. */
int ks_cons_update(ks_cons* c, const char* update_json, size_t len);
/* Host-only: the snapshot with update_json applied ("{}" for none, an array for a sequence), as ks_cons_inspect plus
 * "nodeRows" {name: {available (device units), pods}} for every active node and "poolRemaining". */
int ks_cons_inspect_update(const char* snapshot_json, size_t len, const char* update_json, size_t ulen,
                           char** out_json);
void ks_cons_free(ks_cons* c);
int ks_cons_num_candidates(const ks_cons* c);
int ks_cons_num_sims(const ks_cons* c);
int ks_cons_record_bytes(const ks_cons* c);           /* fixed size of one simulation record */
int ks_cons_records_per_rank(const ks_cons* c, int world);
/* Run the simulations s with s % world == rank on the current (or opts->device) GPU and write their
 * records, in order of s, to `records` (records_per_rank * record_bytes bytes; a device pointer when
 * records_on_device, so an all-gather over RCCL can collect them).  kernel_ms: HIP-event time of the
 * queue sort + simulation kernel on the stream they ran on. */
int ks_cons_run(ks_cons* c, int rank, int world, const ks_solve_opts* opts, void* records, int records_on_device,
                double* kernel_ms);
/* records may be NULL at world 1 (records_on_device 0): the records stay in the handle's pinned host buffer
 * until its next run, and ks_cons_decide / ks_cons_needed_sims / ks_cons_records_alg_bytes take records NULL
 * to read them there (no copy of the pass's records). */
/* Replay the reference's sequential choice over the gathered records ([rank][slot] layout):
 * JSON {"candidates":[{name, disruptionCost}], "multi":{"command", "sims", "path"}, "single":{"command", "sims"}}
 * ("path": the binary search's probes {mid, carried, action}: carried = re-run from pod objects an earlier probe relaxed).
 * flags: KS_CONS_ALL_SIMS reports every simulation (otherwise only those the reference would have
 * run); KS_CONS_CANDIDATES includes the candidate list (otherwise "candidates" is empty).
 * Requirement records (NewNodeClaims[0].Requirements) stay on the GPU that ran a simulation:
 * ks_cons_needed_sims lists (returns the count; writes up to cap) the simulations the output needs,
 * their owners (rank = sim % world) read them with ks_cons_claim_requirements (requirement_words
 * uint32 each), and rs_table passes them to ks_cons_decide in that order.  rs_table may be NULL when world is 1
 * and this handle's last ks_cons_run covered every simulation: the records are then read from that run. */
#define KS_CONS_ALL_SIMS 1   /* flags: report every simulation */
#define KS_CONS_CANDIDATES 2 /* flags: include the ordered candidate list */
#define KS_CONS_NO_SIMS 4    /* flags: leave out the per-simulation "sims" lists (the commands are unchanged) */
int ks_cons_requirement_words(const ks_cons* c);
int ks_cons_needed_sims(ks_cons* c, const void* records, int world, int flags, int32_t* out, int cap);
int ks_cons_claim_requirements(ks_cons* c, int sim, uint32_t* out);
int ks_cons_decide(ks_cons* c, const void* records, int world, int flags, const uint32_t* rs_table,
                   char** json_out);
/* Launch lists of a pass (ks_cons_run with opts->launch_lists set): behind the simulations, one more kernel orders
 * the options of every simulation whose action is replace the way NodeClaimTemplate.ToNodeClaim launches the
 * replacement (see ks_results_nodeclaim_launch): the command's instanceTypeOptions (after filterByPrice; after
 * filterOutSameType for a multi-node prefix) priced under NewNodeClaims[0]'s requirements, narrowed to spot where
 * the command's are (consolidation.go:181-188), by (price, name), cut to 100.  The rows stay on the GPU that ran
 * the simulation.  kernel_ms does not include that kernel; ks_cons_launch_ms is its HIP-event time.  The run
 * fails with KS_ERR_UNSUPPORTED / KS_ERR_CAPACITY as a Solve with launch_lists does (a template listing one name
 * twice; a list too long for the LDS).
 * ks_cons_claim_launch: simulation `sim`'s list, read on its owner (rank = sim % world) and checked on the host
 * against the command's option words first (a failed check is KS_ERR_INTERNAL).  instance_types / prices: room for
 * 100 entries; *n = min(*n_options, 100); any out pointer may be NULL.  KS_ERR_ARG when the simulation is not in
 * this handle's last run, when that run did not set launch_lists, and when the simulation's action is not replace.
 * ks_cons_decide / ks_cons_decide_clock after such a run: every replace command gains "sim" (the simulation to ask,
 * -1 for a carried probe), and its "replacement" gains "launchInstanceTypes": [names] and "launchPrices": [numbers]
 * when the list is in this handle: at world 1 with rs_table NULL, and at any world for a command chosen from a
 * carried probe (its re-run is local and computes its list with the same kernel). */
int ks_cons_claim_launch(ks_cons* c, int sim, int32_t* instance_types, double* prices, int* n, int* n_options);
/* HIP-event time (milliseconds) of the launch-list kernel of the handle's last ks_cons_run or ks_cons_disrupt; 0
 * when that call did not set launch_lists or its command has no replacement to order (no simulation; no pick). */
double ks_cons_launch_ms(const ks_cons* c);
/* The name of instance type `instance_type` as the launch lists index it (the handle's instanceTypes order, also
 * after a binary load); lives as long as the handle.  NULL out of range and for a handle a failed update left
 * unusable. */
const char* ks_cons_instance_type_name(const ks_cons* c, int instance_type);
/* The methods' timeouts (MultiNodeConsolidationTimeoutDuration = 1 min, multinodeconsolidation.go:34,99-110;
 * SingleNodeConsolidationTimeoutDuration = 3 min, singlenodeconsolidation.go:29,58-65) on a virtual clock
 * that advances sim_seconds per simulation the sequential replay consults: the multi-node search returns
 * its last saved command once the clock passes its timeout, the single-node scan abandons with no command.
 * The GPU has already run every simulation, so sim_seconds models the reference's per-simulation cost
 * (0: no timeout ever fires, which is ks_cons_decide).
 * rs_table is the same table as for ks_cons_decide: its rows are in ks_cons_needed_sims order, and that order
 * does not depend on the clock (ks_cons_needed_sims has none).  A clock only stops the search or the scan early,
 * so the clocked replay reads a subset of those rows; the rows of simulations it never consults are ignored. */
typedef struct ks_cons_clock {
  double multi_timeout_s;
  double single_timeout_s;
  double sim_seconds;
} ks_cons_clock;
int ks_cons_decide_clock(ks_cons* c, const void* records, int world, int flags, const uint32_t* rs_table,
                         const ks_cons_clock* clock, char** json_out);
/* Validation.IsValid after its wait + ValidateCommand (disruption/validation.go:68-180): the handle
 * holds the current cluster snapshot (stateNodes may carry "nominated": Cluster.IsNodeNominated);
 * command_json is a command as ks_cons_decide reports it ({"candidates": [names], "replacement":
 * {"instanceTypeOptions": [...]}} or no "replacement"), computed on an earlier snapshot.  The command's
 * candidates are re-filtered (NewCandidate, PDBs, do-not-disrupt), then re-simulated on the GPU.
 * Writes JSON {"valid": bool, "reason": "" | "candidates-changed" | "candidate-nominated" |
 * "no-candidates" | "pods-unschedulable" | "replacement-not-needed" | "multiple-nodeclaims" |
 * "replacement-needed" | "instance-types-not-subset", "sim": null | {allNonPendingScheduled,
 * newNodeClaims, claim0: {nodePoolName, instanceTypeOptions}}}.  Leaves the pass's plan unchanged. */
int ks_cons_validate(ks_cons* c, const char* command_json, size_t len, const ks_solve_opts* opts, char** json_out);
/* Drift and Expiration (disruption/drift.go, expiration.go), the two other methods that simulate once per
 * candidate.  The snapshot's stateNodes may carry "nodeClaimConditions": [{type, status, lastTransitionTime}]
 * (NodeClaim.Status.Conditions as json.Marshal writes them; Drifted and Expired are read; the "cluster" form takes
 * them from the NodeClaim paired with the node) and a top-level "featureGates": {"drift": bool} (default true).
 * The method's candidates are the NewCandidate nodes that pass its ShouldDisrupt (drift.go:56-59: the gate and
 * Drifted True; expiration.go:61-64: the NodePool's expireAfter is a duration and Expired True) and
 * filterCandidates (PDBs, do-not-disrupt pods), ordered by the condition's lastTransitionTime (sort.Slice
 * emulated exactly); consolidation's own ShouldDisrupt does not apply.  If any candidate has no pods the command
 * is all the empty ones and nothing is launched; otherwise every candidate's single-node simulation runs in a
 * launch of its own on the handle's current state (after ks_cons_update: the updated one) and one more kernel
 * picks the first candidate whose simulation schedules every non-pending pod and exports all its NewNodeClaims.
 * The pass's plan, records and ks_cons_last_routes prefix survive; the method's launch is appended to the routes.
 * No validation follows (the reference has none for these methods).  World 1 only.  opts->lds_budget > 0 caps the
 * simulations' LDS plan.  JSON {"method": "drift" | "expiration", "candidates": [names in order], "command":
 * {"action": "no-op" | "delete" | "replace", "candidates": [names], "replacements": [{nodePoolName,
 * instanceTypeOptions, requests, requirements}]}, "sims": [{candidate, allNonPendingScheduled, newNodeClaims}],
 * "plan": {KO, KL, lds}, "kernel_ms"}; "sims" lists the simulations the reference would have run, up to and
 * including the pick (all of them with KS_CONS_ALL_SIMS in flags).  Requests are canonical Quantity text and the
 * requirements those after FinalizeScheduling (no hostname), as ks_results_json renders a Solve's NodeClaims.  The
 * method's simulations keep no commit log, so without KS_CONS_PLACEMENTS the pods per replacement are not
 * reported, and KS_ERR_UNSUPPORTED is returned when the requests' text would depend on them (pods naming a
 * resource in different quantity formats, only some pods naming it while its sum is zero, or a problem with
 * negative requests); the message names the flag.
 * KS_CONS_PLACEMENTS in flags: when the command is replace, the picked simulation is run once more on an
 * instantiation of the simulation kernel that stores its commit log (single-wave; one launch, in a launch of its
 * own, appended to ks_cons_last_routes as "sims_log" / "sims_topo_log").  The re-run's record must equal the
 * picked simulation's in every word a simulation writes, its log must place every pod at most once and agree with the device's pod
 * count per NodeClaim and with the requests the device summed (a miss is KS_ERR_INTERNAL).  Every entry of
 * "replacements" then gains "pods": [uid, ...] in commit order (NodeClaim.Pods), its "requests" are the Merge
 * replayed over those pods with their recorded quantity formats (exact for mixed formats, partly named resources and
 * negative requests: none of the three refusals applies), and the document gains "placements_ms", the HIP-event
 * time of the re-run, before "kernel_ms".  delete and no-op commands launch nothing extra ("placements_ms": 0).
 * Without the flag the document is byte for byte what it was.  opts->launch_lists may be combined with it. */
#define KS_DISRUPT_EXPIRATION 1
#define KS_DISRUPT_DRIFT 2
#define KS_CONS_PLACEMENTS 8 /* flags of ks_cons_disrupt: pods per replacement, requests rendered from the commit log */
/* With opts->launch_lists set every entry of "replacements" also carries "launchInstanceTypes" / "launchPrices":
 * its launch list, computed by a kernel enqueued behind the pick (no host round trip between them) and checked on
 * the host.  The refusals are ks_cons_run's.  The all-empty and no-pick commands have no replacement. */
int ks_cons_disrupt(ks_cons* c, int method, const ks_solve_opts* opts, int flags, char** json_out);
/* Replacement i of the handle's last ks_cons_disrupt, as ks_results_nodeclaim_launch hands out a Solve's: the
 * arrays live until the handle's next ks_cons_disrupt.  KS_ERR_ARG for i out of range and when that call did not
 * set launch_lists. */
int ks_cons_disrupt_launch(const ks_cons* c, int i, const int32_t** instance_types, const double** prices, int* n,
                           int* n_options);
/* Simulation Results of one simulation of this handle's last ks_cons_run: the simulation is run once more with its
 * commit log (as KS_CONS_PLACEMENTS does, with the same checks against the record the run left) and rendered as
 * {"sim", "candidates": [names], "allNonPendingScheduled", "newNodeClaims": [{nodePoolName, instanceTypeOptions,
 * requests, requirements, pods: [uid, ...]}], "existingNodes": [{name, pods: [uid, ...]}], "unscheduled": [uid, ...],
 * "kernel_ms"}.  newNodeClaims are in the Solve's final order with pods in commit order; instanceTypeOptions,
 * requests and requirements are as ks_results_json renders a Solve's NodeClaims after FinalizeScheduling;
 * existingNodes lists only the nodes that received pods, in calculateExistingNodeClaims order; unscheduled are the
 * simulation's pods (pending, then the candidates', then the deleting nodes') that no target holds.  No pod error
 * texts.  `sim` indexes the handle's simulations, [0, ks_cons_num_sims): the multi-node prefixes first, largest
 * first (the prefix of the first m candidates, m >= 2, is simulation num_sims - num_candidates - (m - 1)), then
 * one per candidate in disruption-cost order (candidate i is simulation num_sims - num_candidates + i); it is the
 * "sim" a replace command carries after a launch_lists run.  A command chosen from a carried multi-node probe
 * ("sim": -1) has no simulation in the run and is out of scope.  opts: device and lds_budget (0: automatic).
 * KS_ERR_ARG before the handle's first ks_cons_run, after a ks_cons_update until the next run, for a simulation the
 * last run did not cover (another rank's) and for sim out of range.  The pass's plan and records survive; the
 * launch is appended to ks_cons_last_routes ("family": "sims_log" or "sims_topo_log").  Free json_out with ks_free. */
int ks_cons_sim_results(ks_cons* c, int sim, const ks_solve_opts* opts, char** json_out);
/* Host-only, no device: {"method", "candidates": [names in the method's order], "empty": [the empty ones],
 * "transitionTimes": [seconds]} of the snapshot with update_json applied (NULL or "{}": none; an array: a sequence). */
int ks_cons_inspect_disrupt(const char* snapshot_json, size_t len, const char* update_json, size_t ulen, int method,
                            char** out_json);
/* Host-only: the bytes ks_cons_save writes for a handle of this snapshot, and ks_cons_inspect_disrupt of a handle
 * loaded from such bytes (resaved, optional: that handle saved again; free both with ks_free). */
int ks_cons_encode_binary(const char* snapshot_json, size_t len, void** buf, size_t* buf_len);
int ks_cons_inspect_disrupt_binary(const void* buf, size_t len, int method, char** out_json, void** resaved,
                                   size_t* resaved_len);
/* Diagnostics: the 24 solve counters of simulation `sim` in the last ks_cons_run of this handle. */
int ks_cons_sim_counters(ks_cons* c, int sim, int64_t* out24);
/* The same for up to n counters (27 in this build: + runs of identical pods, pods they placed, exact claim
 * re-sorts); n larger than the build's count copies that count. Returns the number copied or a negative
 * KS_ERR_* code. */
int ks_cons_sim_counters_n(ks_cons* c, int sim, int64_t* out, int n);
/* Test and diagnostic entry (see ks_problem_queue_readback).  After a ks_cons_run: the plan's per-entry arrays as they stand on the device (no new launch).  words (free with
 * ks_free): lentries | lentrySim | lpodmap | lrunlen (n int32 each: the pods of every simulation in plan order,
 * their simulation, every simulation's NewQueue order at its CSR offsets, the identical pods left in the run at
 * each sorted entry), then rank (P int32: every pod's position in the cluster's NewQueue order).  meta_json: the
 * document of ks_problem_queue_inputs for the handle's pods plus {"n", "sims", "rbits", "sbits"}.
 * KS_ERR_ARG before the handle's first run. */
int ks_cons_queue_readback(ks_cons* c, char** meta_json, int32_t** words, size_t* n_words);
/* Multi-node probes the last ks_cons_decide / ks_cons_needed_sims ran on this handle's GPU (-1: none resolved).
 * The reference's binary search hands each probe the pod objects the earlier probes relaxed in place
 * (multinodeconsolidation.go:111-114, helpers.go:102-104, preferences.go:60-147): a probe holding such a pod is
 * re-simulated from the carried relaxation states, one launch per probe (typically none). */
int ks_cons_last_reruns(const ks_cons* c);
/* The k_solve launches since this handle's last ks_cons_run began, in order, as a JSON list of
 * {"family": "sims" | "sims_topo" | "sims_mw" | "sims_mixed" | "sims_log" | "sims_topo_log", "rt", "tl", "lean", "n"} (as "stats"."route" of
 * ks_results_json; "sims_mixed" adds "nmw", its leading simulations on 4-wave workgroups): the pass's own
 * launches (two when the long simulations run on a second stream, or a topology plan launches in two phases),
 * then one per carried-probe re-run of ks_cons_decide / ks_cons_needed_sims, per ks_cons_validate, per
 * ks_cons_disrupt (plus its logged re-run, "sims_log" / "sims_topo_log") and per ks_cons_sim_results.
 * Free with ks_free. */
int ks_cons_last_routes(const ks_cons* c, char** json_out);
/* Algorithmic bytes the gathered simulations scanned, summed from their records. */
double ks_cons_records_alg_bytes(const ks_cons* c, const void* records, int world);

/* Cluster-state accounting (pkg/controllers/state: Cluster.UpdateNodeClaim / UpdateNode / UpdatePod,
 * cluster.go:220-512, and the StateNode accessors, statenode.go:110-333): from {"nodeClaims":
 * [v1beta1.NodeClaim], "nodes": [v1.Node], "pods": [v1.Pod], "volumeDrivers": {"ns/pvc": driver},
 * "csiNodes": [storagev1.CSINode]} derive the state the informers converge to, as the snapshot's
 * "stateNodes" array: {name, providerID, hostName, labels, taints, capacity, allocatable, available,
 * podRequests, daemonSetRequests, initialized, ready, markedForDeletion, creationTimestamp,
 * hostPortUsage, volumeUsage, volumeLimits, pods}.  Host-only (no device).  Free with ks_free. */
int ks_cluster_state(const char* cluster_json, size_t len, char** state_nodes_json);

void ks_free(void* p);
const char* ks_last_error(void);
int ks_device_count(void);
const char* ks_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* KARPENTER_AMD_H_ */
