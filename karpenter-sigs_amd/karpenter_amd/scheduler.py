"""ctypes binding of include/karpenter_amd.h, shaped like the reference's scheduling package.

Reference surface (pkg/controllers/provisioning/scheduling/scheduler.go):
    NewScheduler(ctx, kubeClient, nodeClaimTemplates, nodePools, cluster, stateNodes, topology,
                 instanceTypes, daemonSetPods, recorder, opts) *Scheduler        :49-83
    (*Scheduler).Solve(ctx, pods) *Results                                     :140-189
    Results{NewNodeClaims, ExistingNodes, PodErrors}                           :102-106
Here the NewScheduler arguments and the pods travel as one JSON snapshot.
"""
import ctypes
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# KS_LIB_VARIANT=stats loads the diagnostic build with per-phase cycle counters; =asan the ASan + UBSan
# build of the host translation units (make -C karpenter-sigs_amd asan; scripts/asan_cpu_suite.sh); =tsan
# their ThreadSanitizer build (scripts/tsan_cpu_suite.sh).
_VARIANTS = {"stats": "libkarpenter_amd_stats.so", "asan": "libkarpenter_amd_asan.so", "tsan": "libkarpenter_amd_tsan.so"}
_VARIANT = os.environ.get("KS_LIB_VARIANT", "")
_LIB_PATH = os.path.join(_HERE, _VARIANTS.get(_VARIANT, "libkarpenter_amd_%s.so" % _VARIANT if _VARIANT else "libkarpenter_amd.so"))
_lib = None

KS_ERRORS = {-1: "KS_ERR_PARSE", -2: "KS_ERR_UNSUPPORTED", -3: "KS_ERR_CAPACITY", -4: "KS_ERR_HIP",
             -5: "KS_ERR_INTERNAL", -6: "KS_ERR_ARG"}


class KsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s: %s" % (KS_ERRORS.get(code, code), msg))
        self.code = code


class _Opts(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int), ("simulation_mode", ctypes.c_int), ("replicas", ctypes.c_int),
                ("timing_only", ctypes.c_int), ("lds_budget", ctypes.c_int),
                ("launch_lists", ctypes.c_int), ("reserved", ctypes.c_int * 2)]


class _Clock(ctypes.Structure):  # ks_cons_clock
    _fields_ = [("multi_timeout_s", ctypes.c_double), ("single_timeout_s", ctypes.c_double),
                ("sim_seconds", ctypes.c_double)]


def library_path():
    return _LIB_PATH


def lib():
    """Load libkarpenter_amd.so (built in-tree by `make -C karpenter-sigs_amd`)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise KsError(-4, "libkarpenter_amd.so not built (%s); run __graft_entry__.build()" % _LIB_PATH)
    l = ctypes.CDLL(_LIB_PATH)
    vp = ctypes.c_void_p
    l.ks_problem_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_problem_inspect.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_problem_inspect_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_problem_free.argtypes = [vp]
    l.ks_solve.argtypes = [vp, ctypes.POINTER(_Opts), ctypes.POINTER(vp)]
    l.ks_results_free.argtypes = [vp]
    l.ks_results_json.argtypes = [vp, ctypes.POINTER(vp)]
    l.ks_results_kernel_ms.argtypes = [vp]
    l.ks_results_kernel_ms.restype = ctypes.c_double
    l.ks_results_solve_kernel_ms.argtypes = [vp]
    l.ks_results_solve_kernel_ms.restype = ctypes.c_double
    l.ks_results_algorithmic_bytes.argtypes = [vp]
    l.ks_results_algorithmic_bytes.restype = ctypes.c_double
    l.ks_results_feasibility_ms.argtypes = [vp]
    l.ks_results_feasibility_ms.restype = ctypes.c_double
    l.ks_results_feasibility_bytes.argtypes = [vp]
    l.ks_results_feasibility_bytes.restype = ctypes.c_double
    l.ks_results_node_feasibility_ms.argtypes = [vp]
    l.ks_results_node_feasibility_ms.restype = ctypes.c_double
    l.ks_results_node_feasibility_bytes.argtypes = [vp]
    l.ks_results_node_feasibility_bytes.restype = ctypes.c_double
    l.ks_cluster_state.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_free.argtypes = [vp]
    l.ks_problem_save.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    l.ks_problem_create_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_snapshot_check.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    l.ks_problem_encode_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp),
                                           ctypes.POINTER(ctypes.c_size_t)]
    l.ks_problem_check_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    l.ks_problem_feasibility_rows.argtypes = [vp, ctypes.c_int, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                              ctypes.POINTER(ctypes.c_size_t)]
    l.ks_problem_queue_inputs.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_problem_queue_readback.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t),
                                            ctypes.POINTER(ctypes.c_int)]
    l.ks_rec_headers_run.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp, vp, ctypes.POINTER(vp),
                                     ctypes.POINTER(vp)]
    l.ks_cons_save.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    l.ks_cons_create_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
    l.ks_last_error.restype = ctypes.c_char_p
    l.ks_build_info.restype = ctypes.c_char_p
    _lib = l
    return l


def _check(rc):
    if rc != 0:
        raise KsError(rc, lib().ks_last_error().decode())


def _take_str(ptr):
    s = ctypes.cast(ptr, ctypes.c_char_p).value.decode()
    lib().ks_free(ptr)
    return s


def _encode(snapshot):
    return (snapshot if isinstance(snapshot, str) else json.dumps(snapshot)).encode()


def inspect_binary(blob):
    """inspect() of a binary snapshot (save() / encode_binary()), loaded as from_binary() loads it; no device."""
    blob = bytes(blob)
    out = ctypes.c_void_p()
    _check(lib().ks_problem_inspect_binary(blob, len(blob), ctypes.byref(out)))
    return json.loads(_take_str(out))


def _records_buffer(records):
    """A ctypes buffer over gathered records: a run's own buffer (the memoryview run() returns) as is,
    anything else bytes-like copied once."""
    if (isinstance(records, memoryview) and isinstance(records.obj, ctypes.Array)
            and records.nbytes == ctypes.sizeof(records.obj)):  # the whole buffer, not a slice of it
        return records.obj
    return ctypes.create_string_buffer(bytes(records), len(records))


def inspect(snapshot):
    """Encode a snapshot on the host only (no device): universe sizes and layout, for diagnostics."""
    b = _encode(snapshot)
    out = ctypes.c_void_p()
    _check(lib().ks_problem_inspect(b, len(b), ctypes.byref(out)))
    return json.loads(_take_str(out))


def queue_inputs(snapshot):
    """Host-only (ks_problem_queue_inputs): the encoded inputs of the queue kernels -- per pod the four sort-key
    components, its request row, first-state words and flags, with skMin / skBits, lean, dupUids and the host
    order when pods tie -- for a reference that reads nothing a kernel wrote."""
    b = _encode(snapshot)
    out = ctypes.c_void_p()
    _check(lib().ks_problem_queue_inputs(b, len(b), ctypes.byref(out)))
    return json.loads(_take_str(out))


def rec_headers_meta():
    """RF_* / CA_* / KE_* of the consolidation records, as the library was built (ks_rec_headers_run's metadata;
    no device)."""
    meta = ctypes.c_void_p()
    _check(lib().ks_rec_headers_run(None, None, 0, 0, None, 0, None, None, None, ctypes.byref(meta)))
    return json.loads(_take_str(meta))


def rec_headers_verdicts(records, tw, tpl_beg):
    """Host-only: per record, the message the host's record check throws ("" when it passes)."""
    import numpy as np

    flat = np.ascontiguousarray(np.array(records, dtype=np.int32))
    ns = np.array([len(records)], dtype=np.int32)
    tb = np.array(tpl_beg, dtype=np.int32)
    verdicts = ctypes.c_void_p()
    _check(lib().ks_rec_headers_run(flat.ctypes.data, ns.ctypes.data, 1, tw, tb.ctypes.data, len(tb) - 1, None, None,
                                    ctypes.byref(verdicts), None))
    return json.loads(_take_str(verdicts))[0]


def rec_headers_run(passes, tw, tpl_beg):
    """Test / diagnostic driver of k_rec_headers (ks_rec_headers_run): `passes` is a list of record batches, each a
    list of records of RF_HDR + 3 * tw int32 words; every pass runs over the same device status words and block
    counter.  Returns per pass (headers as a flat list of ns * RF_HDR ints, [status word 0, status word 1], [the
    host check's message per record, "" when it passes])."""
    import numpy as np

    flat = np.ascontiguousarray(np.array([r for batch in passes for r in batch], dtype=np.int32))
    ns = np.array([len(batch) for batch in passes], dtype=np.int32)
    tb = np.array(tpl_beg, dtype=np.int32)
    rf_hdr = rec_headers_meta()["RF_HDR"]
    assert flat.ndim == 2 and flat.shape[1] == rf_hdr + 3 * tw
    hdr = np.zeros(int(ns.sum()) * rf_hdr, dtype=np.int32)
    status = np.zeros(2 * len(passes), dtype=np.uint64)
    verdicts = ctypes.c_void_p()
    _check(lib().ks_rec_headers_run(flat.ctypes.data, ns.ctypes.data, len(passes), tw, tb.ctypes.data, len(tb) - 1,
                                    hdr.ctypes.data, status.ctypes.data, ctypes.byref(verdicts), None))
    verdicts = json.loads(_take_str(verdicts))
    out, at = [], 0
    for i, n in enumerate(ns):
        out.append(([int(x) for x in hdr[at:at + int(n) * rf_hdr]], [int(status[2 * i]), int(status[2 * i + 1])],
                    verdicts[i]))
        at += int(n) * rf_hdr
    return out


def claim_sort_probe(keys, order, claim_tpl, claim_head, mode=0, pos=-1, device=0, path=False):
    """Test / diagnostic (ks_claim_sort_probe): the Solve kernel's claim re-sort on arrays of the caller's choosing,
    or with device=-1 Go's pdqsort_func on the host.  claim_head is [n][R], R 3 or 4.  Returns (keys, order, ptpl,
    phead, how) as numpy arrays and an int.  path=True (ks_claim_sort_probe_path) appends the general re-sort's path:
    1 finished on the register copy, 3 more entries than the copy holds, 2 abandoned on a failed invariant (2 and 3:
    sorted by the LDS code), 0 neither; device=-3 runs the lane model of the 64-entry copy on the host (-2: of the
    128-entry form), the path then carrying its breakPatterns calls << 8 and heapSort calls << 20."""
    import numpy as np

    k = np.array(keys, dtype=np.int32)
    o = np.array(order, dtype=np.int32)
    ct = np.ascontiguousarray(claim_tpl, dtype=np.int32)
    ch = np.ascontiguousarray(claim_head, dtype=np.int64)
    n = len(k)
    assert len(o) == n and len(ct) == n and ch.ndim == 2 and ch.shape[0] == n
    r = ch.shape[1]
    pt = np.zeros(n, dtype=np.int32)
    ph = np.zeros((n, r), dtype=np.int64)
    how = ctypes.c_int(-1)
    if path or device < -1:
        pth = ctypes.c_int(0)
        lib().ks_claim_sort_probe_path.argtypes = ([ctypes.c_int] * 5 + [ctypes.c_void_p] * 6 +
                                                   [ctypes.POINTER(ctypes.c_int)] * 2)
        _check(lib().ks_claim_sort_probe_path(device, mode, pos, n, r, k.ctypes.data, o.ctypes.data, ct.ctypes.data,
                                              ch.ctypes.data, pt.ctypes.data, ph.ctypes.data, ctypes.byref(how),
                                              ctypes.byref(pth)))
        return (k, o, pt, ph, how.value, pth.value) if path else (k, o, pt, ph, how.value)
    # (bound here, not in lib(): an earlier commit's library, loaded for an A/B run, lacks the entry)
    lib().ks_claim_sort_probe.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 6 + [ctypes.POINTER(ctypes.c_int)]
    _check(lib().ks_claim_sort_probe(device, mode, pos, n, r, k.ctypes.data, o.ctypes.data, ct.ctypes.data,
                                     ch.ctypes.data, pt.ctypes.data, ph.ctypes.data, ctypes.byref(how)))
    return k, o, pt, ph, how.value


def claim_sort_probe_append(keys, order, claim_tpl, claim_head, device=0):
    """Test / diagnostic (ks_claim_sort_probe_append): the re-sort after a claim appended behind greater counts, the
    origin told to the kernel as the Solve tells it; device=-1: Go's pdqsort_func on the host.  Returns (keys, order,
    ptpl, phead, how, taken), taken 1 when the appended claim's closed form ran."""
    import numpy as np

    k = np.array(keys, dtype=np.int32)
    o = np.array(order, dtype=np.int32)
    ct = np.ascontiguousarray(claim_tpl, dtype=np.int32)
    ch = np.ascontiguousarray(claim_head, dtype=np.int64)
    n = len(k)
    assert len(o) == n and len(ct) == n and ch.ndim == 2 and ch.shape[0] == n
    r = ch.shape[1]
    pt = np.zeros(n, dtype=np.int32)
    ph = np.zeros((n, r), dtype=np.int64)
    how, taken = ctypes.c_int(-1), ctypes.c_int(0)
    lib().ks_claim_sort_probe_append.argtypes = ([ctypes.c_int] * 3 + [ctypes.c_void_p] * 6 +
                                                 [ctypes.POINTER(ctypes.c_int)] * 2)
    _check(lib().ks_claim_sort_probe_append(device, n, r, k.ctypes.data, o.ctypes.data, ct.ctypes.data, ch.ctypes.data,
                                            pt.ctypes.data, ph.ctypes.data, ctypes.byref(how), ctypes.byref(taken)))
    return k, o, pt, ph, how.value, taken.value


def cluster_state(cluster):
    """Cluster-state accounting (pkg/controllers/state, cluster.go:220-512 + statenode.go:110-333):
    the StateNode accessor values the informers converge to for {"nodeClaims", "nodes", "pods"}, as a
    snapshot "stateNodes" list (host-only; no device)."""
    b = _encode(cluster)
    out = ctypes.c_void_p()
    _check(lib().ks_cluster_state(b, len(b), ctypes.byref(out)))
    return json.loads(_take_str(out))


class Results:
    """scheduling.Results: new_nodeclaims, existing_nodes, pod_errors (keys = input pod index)."""

    def __init__(self, doc, kernel_ms, alg_bytes, solve_kernel_ms=0.0):
        self.doc = doc
        self.new_nodeclaims = doc["newNodeClaims"]
        self.existing_nodes = doc["existingNodes"]
        self.pod_errors = {int(k): v for k, v in doc["podErrors"].items()}
        self.stats = doc.get("stats", {})
        self.kernel_ms = kernel_ms
        self.solve_kernel_ms = solve_kernel_ms
        self.algorithmic_bytes = alg_bytes
        self.feasibility_ms = 0.0     # k_feasibility inside this Solve (0: not launched)
        self.feasibility_bytes = 0.0  # its algorithmic bytes
        self.node_feasibility_ms = 0.0     # k_feasibility_nodes inside this Solve (0: not launched)
        self.node_feasibility_bytes = 0.0  # its algorithmic bytes

    def canonical(self):
        d = dict(self.doc)
        d.pop("stats", None)
        return d


class _Requirement(ctypes.Structure):  # ks_requirement
    _fields_ = [("key", ctypes.c_char_p), ("op", ctypes.c_char_p), ("n_values", ctypes.c_int),
                ("values", ctypes.POINTER(ctypes.c_char_p)), ("has_gt", ctypes.c_int), ("has_lt", ctypes.c_int),
                ("gt", ctypes.c_int64), ("lt", ctypes.c_int64)]


_accessors_bound = False


def _bind_accessors(l):
    global _accessors_bound
    if _accessors_bound:
        return
    vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
    i32pp = ctypes.POINTER(ctypes.POINTER(ctypes.c_int32))
    strpp = ctypes.POINTER(ctypes.POINTER(ctypes.c_char_p))
    l.ks_results_num_new_nodeclaims.argtypes = [vp]
    l.ks_results_nodeclaim.argtypes = [vp, ctypes.c_int, ip, i32pp, ip, i32pp, ip]
    l.ks_results_nodeclaim_requests.argtypes = [vp, ctypes.c_int, ip, strpp, strpp]
    l.ks_results_nodeclaim_requirements.argtypes = [vp, ctypes.c_int, ip, ctypes.POINTER(ctypes.POINTER(_Requirement))]
    l.ks_results_num_existing_nodes.argtypes = [vp]
    l.ks_results_existing_node.argtypes = [vp, ctypes.c_int, ip, i32pp, ip]
    l.ks_results_num_pod_errors.argtypes = [vp]
    l.ks_results_pod_error.argtypes = [vp, ctypes.c_int, ip, ctypes.POINTER(ctypes.c_char_p)]
    l.ks_results_nodeclaim_launch.argtypes = [vp, ctypes.c_int, i32pp, ctypes.POINTER(ctypes.POINTER(ctypes.c_double)), ip, ip]
    l.ks_results_launch_ms.argtypes = [vp]
    l.ks_results_launch_ms.restype = ctypes.c_double
    _accessors_bound = True


class StructuredResults:
    """Results read through the C-ABI's structured accessors (what the cgo shim in INTEGRATION.md does):
    new_nodeclaims = [{template, pods, instance_types (indices), requests {name: quantity},
    requirements [(key, op, values, gt, lt)]}], existing_nodes = [(state node index, pods)],
    pod_errors = {pod index: message}.  After solve_structured(launch_lists=True) every claim also carries
    launch (instance-type names in OrderByPrice order, the first 100), launch_prices (the price that ordered each)
    and n_options, and launch_ms is the launch-list kernel's time; otherwise the claims have no such keys and
    launch_ms is 0."""

    def __init__(self, claims, nodes, errors, kernel_ms, solve_kernel_ms, launch_ms=0.0):
        self.new_nodeclaims = claims
        self.existing_nodes = nodes
        self.pod_errors = errors
        self.kernel_ms = kernel_ms
        self.solve_kernel_ms = solve_kernel_ms
        self.launch_ms = launch_ms


def _read_structured(l, r, launch_names=None):
    """launch_names: the snapshot's instance-type names when the Solve set launch_lists (None: no launch data)."""
    import numpy as np

    _bind_accessors(l)
    tpl, n1, n2 = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    a1, a2 = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_int32)()
    claims = []
    for i in range(l.ks_results_num_new_nodeclaims(r)):
        _check(l.ks_results_nodeclaim(r, i, ctypes.byref(tpl), ctypes.byref(a1), ctypes.byref(n1), ctypes.byref(a2),
                                      ctypes.byref(n2)))
        pods = np.ctypeslib.as_array(a1, (n1.value,)).copy() if n1.value else np.zeros(0, np.int32)
        its = np.ctypeslib.as_array(a2, (n2.value,)).copy() if n2.value else np.zeros(0, np.int32)
        names, qtys = ctypes.POINTER(ctypes.c_char_p)(), ctypes.POINTER(ctypes.c_char_p)()
        _check(l.ks_results_nodeclaim_requests(r, i, ctypes.byref(n1), ctypes.byref(names), ctypes.byref(qtys)))
        requests = {names[k].decode(): qtys[k].decode() for k in range(n1.value)}
        rq = ctypes.POINTER(_Requirement)()
        _check(l.ks_results_nodeclaim_requirements(r, i, ctypes.byref(n1), ctypes.byref(rq)))
        reqs = []
        for k in range(n1.value):
            x = rq[k]
            reqs.append((x.key.decode(), x.op.decode(), [x.values[v].decode() for v in range(x.n_values)],
                         x.gt if x.has_gt else None, x.lt if x.has_lt else None))
        claims.append({"template": tpl.value, "pods": pods, "instance_types": its, "requests": requests,
                       "requirements": reqs})
        if launch_names is not None:
            pr = ctypes.POINTER(ctypes.c_double)()
            _check(l.ks_results_nodeclaim_launch(r, i, ctypes.byref(a1), ctypes.byref(pr), ctypes.byref(n1), ctypes.byref(n2)))
            claims[-1]["launch"] = [launch_names[a1[k]] for k in range(n1.value)]
            claims[-1]["launch_prices"] = [pr[k] for k in range(n1.value)]
            claims[-1]["n_options"] = n2.value
    nodes = []
    for i in range(l.ks_results_num_existing_nodes(r)):
        _check(l.ks_results_existing_node(r, i, ctypes.byref(n2), ctypes.byref(a1), ctypes.byref(n1)))
        pods = np.ctypeslib.as_array(a1, (n1.value,)).copy() if n1.value else np.zeros(0, np.int32)
        nodes.append((n2.value, pods))
    errors = {}
    msg = ctypes.c_char_p()
    for i in range(l.ks_results_num_pod_errors(r)):
        _check(l.ks_results_pod_error(r, i, ctypes.byref(n1), ctypes.byref(msg)))
        errors[n1.value] = msg.value.decode()
    return claims, nodes, errors


def _take_bytes(fn, handle):
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(fn(handle, ctypes.byref(buf), ctypes.byref(n)))
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        lib().ks_free(buf)


def snapshot_check(snapshot):
    """Host-only: encode, save, load, save again; raises unless the two snapshots are byte-identical.
    Returns the snapshot size in bytes."""
    b = _encode(snapshot)
    n = ctypes.c_size_t()
    _check(lib().ks_snapshot_check(b, len(b), ctypes.byref(n)))
    return n.value


def encode_binary(snapshot):
    """Host-only: the binary snapshot of a JSON problem (what Scheduler(snapshot).save() returns), no device."""
    b = _encode(snapshot)
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(lib().ks_problem_encode_binary(b, len(b), ctypes.byref(buf), ctypes.byref(n)))
    try:
        return ctypes.string_at(buf, n.value)
    finally:
        lib().ks_free(buf)


def check_binary(blob):
    """Host-only: ks_problem_create_binary's load-time checks; raises KsError (KS_ERR_PARSE) on a bad blob."""
    blob = bytes(blob)
    _check(lib().ks_problem_check_binary(blob, len(blob)))


class StaticFeasibility:
    """The static feasibility matrix (ks_problem_static_feasibility): numpy arrays tpl_code[S, NTPL],
    tpl_count[S, NTPL], tpl_options[S, NTPL, TW], node_bits[S, NWN], node_count[S], the meta document that
    indexes them, and the timing (kernel_ms, templates_ms, nodes_ms, bytes_read, bytes_written).  A clear bit
    holds for every Solve of the problem; a set one is exact for an empty scheduler without topology and volume
    limits (meta["ignores"])."""

    def __init__(self, meta, arrays, timing):
        self.meta = meta
        self.tpl_code, self.tpl_count, self.tpl_options, self.node_bits, self.node_count = arrays
        self.kernel_ms, self.templates_ms, self.nodes_ms, self.bytes_read, self.bytes_written = timing
        self.codes = meta["codes"]

    def state(self, pod, state=0):
        """The row index of `pod`'s relaxation state number `state` (0: unrelaxed)."""
        if not 0 <= pod < len(self.meta["podState0"]) or not 0 <= state < self.meta["podNState"][pod]:
            raise IndexError("pod %d has no relaxation state %d" % (pod, state))
        return self.meta["podState0"][pod] + state

    def states(self, pod):
        s0 = self.state(pod, 0)
        return range(s0, s0 + self.meta["podNState"][pod])

    def options(self, pod, state, tpl):
        """Names of the instance types a fresh NodeClaim of template `tpl` keeps for the pod in that state."""
        names = self.meta["templates"][tpl]["instanceTypes"]
        words = self.tpl_options[self.state(pod, state), tpl]
        return [n for q, n in enumerate(names) if (int(words[q >> 5]) >> (q & 31)) & 1]

    def nodes(self, pod, state):
        """Names of the existing nodes that accept the pod in that state."""
        words = self.node_bits[self.state(pod, state)]
        return [n for i, n in enumerate(self.meta["nodes"]) if (int(words[i >> 5]) >> (i & 31)) & 1]

    def unschedulable(self):
        """{pod: [code per template, of its last state]} for the pods with no option and no node in any state of
        their chain: no Solve of this problem schedules them.  Pods with a state in meta["undefinedKeyStates"] are
        left out: their clear bits hold for a fresh NodeClaim or an untouched node only (a target gains label keys
        as other pods land on it)."""
        out = {}
        soft = set(self.meta["undefinedKeyStates"])
        for pod in range(len(self.meta["podState0"])):
            ss = self.states(pod)
            if soft.intersection(ss):
                continue
            if not any(self.tpl_count[s].any() or self.node_count[s] for s in ss):
                out[pod] = [int(c) for c in self.tpl_code[ss[-1]]]
        return out


class Scheduler:
    """NewScheduler(...) on the GPU: the snapshot is encoded once and stays resident in HBM.
    Scheduler.from_binary(blob) rebuilds one from save()'s binary snapshot (no JSON parse, no encode)."""

    def __init__(self, snapshot, _binary=None, _host_only=False):
        h = ctypes.c_void_p()
        # launch lists are reported by name: the names are read from the snapshot on first use (a reference, no copy)
        self._snapshot, self._it_names = snapshot, None
        if _host_only:
            b = _encode(snapshot)
            lib().ks_problem_create_host.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_void_p)]
            _check(lib().ks_problem_create_host(b, len(b), ctypes.byref(h)))
        elif _binary is not None:
            _check(lib().ks_problem_create_binary(_binary, len(_binary), ctypes.byref(h)))
        else:
            b = _encode(snapshot)
            _check(lib().ks_problem_create(b, len(b), ctypes.byref(h)))
        self._h = h

    @classmethod
    def from_binary(cls, blob):
        return cls(None, _binary=bytes(blob))

    @classmethod
    def host_only(cls, snapshot):
        """The encoded problem without a device (ks_problem_create_host): static_feasibility(where="host") and
        save() work on it, solve() raises KS_ERR_HIP."""
        return cls(snapshot, _host_only=True)

    def save(self):
        """The binary snapshot of the encoded problem (bytes)."""
        return _take_bytes(lib().ks_problem_save, self._h)

    def static_feasibility(self, where="device", device=-1):
        """Every relaxation state against every template's instance types and every existing node, from the
        static tables alone (ks_problem_static_feasibility): a StaticFeasibility.  where="device" runs the two
        kernels, where="host" the same definitions in plain loops on the host."""
        import numpy as np

        if where not in ("device", "host"):
            raise KsError(-6, 'where must be "device" or "host"')
        l = lib()
        vp, c = ctypes.c_void_p, ctypes
        l.ks_problem_static_feasibility.argtypes = [vp, c.POINTER(_Opts), c.c_int, c.POINTER(vp)]
        l.ks_feasibility_free.argtypes = [vp]
        l.ks_feasibility_meta.argtypes = [vp, c.POINTER(vp)]
        l.ks_feasibility_arrays.argtypes = [vp, c.POINTER(c.c_int), c.POINTER(vp), c.POINTER(vp), c.POINTER(vp),
                                            c.POINTER(vp), c.POINTER(vp)]
        l.ks_feasibility_timing.argtypes = [vp, c.POINTER(c.c_double), c.POINTER(c.c_int64), c.POINTER(c.c_int64)]
        l.ks_feasibility_kernel_times.argtypes = [vp, c.POINTER(c.c_double), c.POINTER(c.c_double)]
        o = _Opts(device, 1, 1, 0, 0)
        f = vp()
        _check(l.ks_problem_static_feasibility(self._h, c.byref(o), 1 if where == "host" else 0, c.byref(f)))
        try:
            meta = vp()
            _check(l.ks_feasibility_meta(f, c.byref(meta)))
            meta = json.loads(_take_str(meta))
            dims = (c.c_int * 5)()
            ptr = [vp() for _ in range(5)]
            _check(l.ks_feasibility_arrays(f, dims, *[c.byref(x) for x in ptr]))
            S, NTPL, _, TW, NWN = list(dims)
            shapes = [((S, NTPL), np.uint32), ((S, NTPL), np.int32), ((S, NTPL, TW), np.uint32), ((S, NWN), np.uint32),
                      ((S,), np.int32)]
            arrays = []
            for x, (shape, dt) in zip(ptr, shapes):
                n = int(np.prod(shape))
                raw = c.string_at(x, n * 4) if n else b""
                arrays.append(np.frombuffer(raw, dtype=dt).reshape(shape).copy())
            ms, tms, nms = c.c_double(), c.c_double(), c.c_double()
            br, bw = c.c_int64(), c.c_int64()
            _check(l.ks_feasibility_timing(f, c.byref(ms), c.byref(br), c.byref(bw)))
            _check(l.ks_feasibility_kernel_times(f, c.byref(tms), c.byref(nms)))
            return StaticFeasibility(meta, arrays, (ms.value, tms.value, nms.value, br.value, bw.value))
        finally:
            l.ks_feasibility_free(f)

    def feasibility_rows(self, which):
        """Test / diagnostic read-back (ks_problem_feasibility_rows): which = 0 the pod-state x instance-type
        rows, 1 the pod-state x existing-node rows, as the kernels a Solve launches write them.  Returns
        (meta dict, words as a numpy uint32 array); KsError KS_ERR_UNSUPPORTED when the table is off."""
        import numpy as np

        meta, words, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(lib().ks_problem_feasibility_rows(self._h, which, ctypes.byref(meta), ctypes.byref(words), ctypes.byref(n)))
        try:
            arr = np.frombuffer(ctypes.string_at(words, n.value * 4), dtype=np.uint32).copy()
        finally:
            lib().ks_free(words)
        return json.loads(_take_str(meta)), arr

    def queue_readback(self):
        """Test / diagnostic read-back (ks_problem_queue_readback): the queue launches a Solve makes before k_solve.
        Returns (order, run lengths or None when the problem is not lean, whether the device sort produced the
        order), the arrays as lists of P ints."""
        import numpy as np

        order, rl, n, dev = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_int()
        _check(lib().ks_problem_queue_readback(self._h, ctypes.byref(order), ctypes.byref(rl), ctypes.byref(n),
                                               ctypes.byref(dev)))
        try:
            o = np.frombuffer(ctypes.string_at(order, n.value * 4), dtype=np.int32).tolist()
            r = np.frombuffer(ctypes.string_at(rl, n.value * 4), dtype=np.int32).tolist() if rl.value else None
        finally:
            lib().ks_free(order)
            if rl.value:
                lib().ks_free(rl)
        return o, r, bool(dev.value)

    def solve(self, replicas=1, device=-1, simulation_mode=True, timing_only=False, lds_budget=0):
        """Solve(ctx, pods) with fresh scheduler state; replicas>1 runs that many independent copies
        of the same Solve in one launch (one wavefront each) and returns replica 0's results."""
        o = _Opts(device, 1 if simulation_mode else 0, replicas, 1 if timing_only else 0, lds_budget)
        r = ctypes.c_void_p()
        _check(lib().ks_solve(self._h, ctypes.byref(o), ctypes.byref(r)))
        try:
            if timing_only:
                out = Results({"newNodeClaims": [], "existingNodes": [], "podErrors": {}},
                              lib().ks_results_kernel_ms(r), lib().ks_results_algorithmic_bytes(r),
                              lib().ks_results_solve_kernel_ms(r))
            else:
                js = ctypes.c_void_p()
                _check(lib().ks_results_json(r, ctypes.byref(js)))
                doc = json.loads(_take_str(js))
                out = Results(doc, lib().ks_results_kernel_ms(r), lib().ks_results_algorithmic_bytes(r),
                              lib().ks_results_solve_kernel_ms(r))
            out.feasibility_ms = lib().ks_results_feasibility_ms(r)
            out.feasibility_bytes = lib().ks_results_feasibility_bytes(r)
            out.node_feasibility_ms = lib().ks_results_node_feasibility_ms(r)
            out.node_feasibility_bytes = lib().ks_results_node_feasibility_bytes(r)
            return out
        finally:
            lib().ks_results_free(r)

    def _instance_type_names(self):
        if self._it_names is None:
            if self._snapshot is None:
                raise KsError(-6, "launch lists by name need the JSON snapshot the Scheduler was created from")
            doc = self._snapshot if isinstance(self._snapshot, dict) else json.loads(self._snapshot)
            self._it_names = [it["name"] for it in doc.get("instanceTypes", [])]
            self._snapshot = None
        return self._it_names

    def solve_structured(self, device=-1, simulation_mode=True, launch_lists=False, lds_budget=0, with_json=False):
        """Solve(ctx, pods) with the Results read through the structured accessors (no JSON): the drop-in
        caller's full return path (INTEGRATION.md's cgo shim).  launch_lists: every claim also carries its launch
        list (ks_results_nodeclaim_launch), computed on the device.  with_json: the same Results' ks_results_json
        document as .doc (tests compare the two)."""
        l = lib()
        names = self._instance_type_names() if launch_lists else None
        o = _Opts(device, 1 if simulation_mode else 0, 1, 0, lds_budget, 1 if launch_lists else 0)
        r = ctypes.c_void_p()
        _check(l.ks_solve(self._h, ctypes.byref(o), ctypes.byref(r)))
        try:
            claims, nodes, errors = _read_structured(l, r, names)
            out = StructuredResults(claims, nodes, errors, l.ks_results_kernel_ms(r), l.ks_results_solve_kernel_ms(r),
                                    l.ks_results_launch_ms(r))
            if with_json:
                js = ctypes.c_void_p()
                _check(l.ks_results_json(r, ctypes.byref(js)))
                out.doc = json.loads(_take_str(js))
            return out
        finally:
            l.ks_results_free(r)

    def timed_collect(self, steps, device=-1, simulation_mode=True):
        """Mean ms of `steps` ks_solve calls with the Results collected (no accessor walk) + ks_results_free:
        the C-ABI cost of the drop-in return path, without Python's per-field ctypes overhead."""
        import time
        l = lib()
        o = _Opts(device, 1 if simulation_mode else 0, 1, 0, 0)
        r = ctypes.c_void_p()
        t = time.perf_counter()
        for _ in range(steps):
            _check(l.ks_solve(self._h, ctypes.byref(o), ctypes.byref(r)))
            l.ks_results_free(r)
        return (time.perf_counter() - t) * 1000.0 / steps

    def close(self):
        if self._h:
            lib().ks_problem_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _cons_lib():
    l = lib()
    if not getattr(l, "_cons_ready", False):
        vp = ctypes.c_void_p
        l.ks_cons_create.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
        l.ks_cons_free.argtypes = [vp]
        l.ks_cons_inspect.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp)]
        l.ks_cons_inspect_update.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                             ctypes.POINTER(vp)]
        l.ks_cons_update.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t]
        for f in ("ks_cons_num_candidates", "ks_cons_num_sims", "ks_cons_record_bytes"):
            getattr(l, f).argtypes = [vp]
        l.ks_cons_records_per_rank.argtypes = [vp, ctypes.c_int]
        l.ks_cons_run.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_Opts), vp, ctypes.c_int,
                                  ctypes.POINTER(ctypes.c_double)]
        l.ks_cons_decide.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(vp)]
        l.ks_cons_decide_clock.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, vp, ctypes.POINTER(_Clock), ctypes.POINTER(vp)]
        l.ks_cons_requirement_words.argtypes = [vp]
        l.ks_cons_needed_sims.argtypes = [vp, vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
        l.ks_cons_claim_requirements.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32)]
        l.ks_cons_validate.argtypes = [vp, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(_Opts), ctypes.POINTER(vp)]
        l.ks_cons_sim_counters.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        l.ks_cons_sim_counters_n.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.c_int]
        l.ks_cons_records_alg_bytes.argtypes = [vp, vp, ctypes.c_int]
        l.ks_cons_records_alg_bytes.restype = ctypes.c_double
        l.ks_cons_last_reruns.argtypes = [vp]
        l.ks_cons_last_reruns.restype = ctypes.c_int
        l.ks_cons_last_routes.argtypes = [vp, ctypes.POINTER(vp)]
        l.ks_cons_disrupt.argtypes = [vp, ctypes.c_int, ctypes.POINTER(_Opts), ctypes.c_int, ctypes.POINTER(vp)]
        l.ks_cons_sim_results.argtypes = [vp, ctypes.c_int, ctypes.POINTER(_Opts), ctypes.POINTER(vp)]
        l.ks_cons_claim_launch.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                                           ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        l.ks_cons_disrupt_launch.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.POINTER(ctypes.c_int32)),
                                             ctypes.POINTER(ctypes.POINTER(ctypes.c_double)), ctypes.POINTER(ctypes.c_int),
                                             ctypes.POINTER(ctypes.c_int)]
        l.ks_cons_launch_ms.argtypes = [vp]
        l.ks_cons_launch_ms.restype = ctypes.c_double
        l.ks_cons_instance_type_name.argtypes = [vp, ctypes.c_int]
        l.ks_cons_instance_type_name.restype = ctypes.c_char_p
        l.ks_cons_inspect_disrupt.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_size_t,
                                              ctypes.c_int, ctypes.POINTER(vp)]
        l.ks_cons_encode_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(vp),
                                            ctypes.POINTER(ctypes.c_size_t)]
        l.ks_cons_inspect_disrupt_binary.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(vp),
                                                     ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        l.ks_cons_queue_readback.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
        l._cons_ready = True
    return l


def inspect_consolidation(snapshot):
    """Host-only: the ordered candidates and the simulation plan of a cluster snapshot."""
    b = _encode(snapshot)
    out = ctypes.c_void_p()
    _check(_cons_lib().ks_cons_inspect(b, len(b), ctypes.byref(out)))
    return json.loads(_take_str(out))


def inspect_consolidation_update(snapshot, update=None):
    """Host-only: the snapshot with a ks_cons_update delta applied (None: as it is), with every active
    node's encoded available row and pods and the pools' remaining limits ("nodeRows", "poolRemaining")."""
    b = _encode(snapshot)
    u = _encode(update if update is not None else {})
    out = ctypes.c_void_p()
    _check(_cons_lib().ks_cons_inspect_update(b, len(b), u, len(u), ctypes.byref(out)))
    return json.loads(_take_str(out))


DISRUPT_METHODS = {"expiration": 1, "drift": 2}  # KS_DISRUPT_EXPIRATION / KS_DISRUPT_DRIFT
KS_CONS_PLACEMENTS = 8  # ks_cons_disrupt flag: pods per replacement, requests rendered from the commit log


def _method(method):
    return DISRUPT_METHODS[method] if isinstance(method, str) else int(method)


def inspect_disruption(snapshot, method, update=None):
    """Host-only: the candidates of Drift / Expiration ("drift" | "expiration") in the method's order and the
    empty ones, for the snapshot with a ks_cons_update delta (or a list of them) applied:
    {"method", "candidates", "empty", "transitionTimes"}."""
    b = _encode(snapshot)
    u = None if update is None else _encode(update)
    out = ctypes.c_void_p()
    _check(_cons_lib().ks_cons_inspect_disrupt(b, len(b), u, len(u) if u else 0, _method(method), ctypes.byref(out)))
    return json.loads(_take_str(out))


def encode_consolidation_binary(snapshot):
    """Host-only: the bytes Consolidator(snapshot).save() writes (no device)."""
    l = _cons_lib()
    b = _encode(snapshot)
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check(l.ks_cons_encode_binary(b, len(b), ctypes.byref(buf), ctypes.byref(n)))
    blob = ctypes.string_at(buf, n.value)
    l.ks_free(buf)
    return blob


def inspect_disruption_binary(blob, method):
    """Host-only: inspect_disruption of the handle a binary snapshot loads to; returns (doc, that handle's
    save() bytes)."""
    l = _cons_lib()
    blob = bytes(blob)
    out, buf, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    _check(l.ks_cons_inspect_disrupt_binary(blob, len(blob), _method(method), ctypes.byref(out), ctypes.byref(buf),
                                            ctypes.byref(n)))
    again = ctypes.string_at(buf, n.value)
    l.ks_free(buf)
    return json.loads(_take_str(out)), again


def shard_slot(sim, world):
    """Where simulation `sim` lands in the [rank][slot] gather (ks_cons_run / ks_cons_decide)."""
    return sim % world, sim // world


class Consolidator:
    """One disruption pass of consolidation on the GPU (pkg/controllers/disruption).

    Mirrors MultiNodeConsolidation / SingleNodeConsolidation.ComputeCommand over a cluster snapshot
    (INTEGRATION.md §5): every candidate-deletion simulation (simulateScheduling, helpers.go:73-127)
    runs on the GPU with its computeConsolidation decision; `decide` replays the reference's
    sequential choice.  Sharding: rank r of `world` runs simulations s with s % world == r."""

    def __init__(self, snapshot, _binary=None):
        l = _cons_lib()
        h = ctypes.c_void_p()
        if _binary is not None:
            _check(l.ks_cons_create_binary(_binary, len(_binary), ctypes.byref(h)))
        else:
            b = _encode(snapshot)
            _check(l.ks_cons_create(b, len(b), ctypes.byref(h)))
        self._h = h
        self.num_candidates = l.ks_cons_num_candidates(h)
        self.num_sims = l.ks_cons_num_sims(h)
        self.record_bytes = l.ks_cons_record_bytes(h)
        self.requirement_words = l.ks_cons_requirement_words(h)

    @classmethod
    def from_binary(cls, blob):
        """A handle from save()'s binary snapshot (host model + candidates + simulation plan)."""
        return cls(None, _binary=bytes(blob))

    def save(self):
        return _take_bytes(_cons_lib().ks_cons_save, self._h)

    def records_per_rank(self, world=1):
        return _cons_lib().ks_cons_records_per_rank(self._h, world)

    def update(self, delta):
        """Cluster-state events since the snapshot or the last update (ks_cons_update):
        {"deletePods": [uid], "bindPods": [{"uid", "node"}], "removeNodes": [name]}.  The next run()
        simulates the updated cluster; the candidate and simulation counts are refreshed."""
        l = _cons_lib()
        b = _encode(delta)
        _check(l.ks_cons_update(self._h, b, len(b)))
        self.num_candidates = l.ks_cons_num_candidates(self._h)
        self.num_sims = l.ks_cons_num_sims(self._h)
        self._recbuf = None

    def run(self, rank=0, world=1, device=-1, out_ptr=None, keep=False, launch_lists=False):
        """Run this rank's simulations.  launch_lists: also compute the launch list of every simulation whose
        action is replace (claim_launch; decide() then reports them with the commands).  out_ptr: device pointer for records_per_rank*record_bytes
        bytes (e.g. a torch tensor's data_ptr()); None returns the records in host memory.
        Returns (records or None, kernel ms).

        The host records are a memoryview over one buffer per handle that every run() of the handle
        overwrites (no copy per pass): a caller keeping one pass's records across the next run() must copy
        them (bytes(records))."""
        l = _cons_lib()
        o = _Opts(device, 1, 1, 0, 0, 1 if launch_lists else 0)
        ms = ctypes.c_double()
        if keep:  # world 1: the records stay in the handle's pinned buffer; pass records=None to decide()
            _check(l.ks_cons_run(self._h, rank, world, ctypes.byref(o), None, 0, ctypes.byref(ms)))
            return None, ms.value
        if out_ptr is None:
            # one host buffer per handle, reused by every pass and handed on without copies (a memoryview,
            # valid until the handle's next run; bytes(view) keeps a copy)
            n = self.records_per_rank(world) * self.record_bytes
            if getattr(self, "_recbuf", None) is None or len(self._recbuf) != n:
                self._recbuf = ctypes.create_string_buffer(n)
            _check(l.ks_cons_run(self._h, rank, world, ctypes.byref(o), ctypes.cast(self._recbuf, ctypes.c_void_p), 0,
                                 ctypes.byref(ms)))
            return memoryview(self._recbuf), ms.value
        _check(l.ks_cons_run(self._h, rank, world, ctypes.byref(o), ctypes.c_void_p(out_ptr), 1, ctypes.byref(ms)))
        return None, ms.value

    def needed_sims(self, records, world=1, all_sims=False):  # noqa: D401
        """Simulations whose NewNodeClaims[0] requirements the decision output needs (in order)."""
        l = _cons_lib()
        buf = _records_buffer(records)
        cap = 64
        while True:
            out = (ctypes.c_int32 * cap)()
            n = l.ks_cons_needed_sims(self._h, ctypes.cast(buf, ctypes.c_void_p), world, 1 if all_sims else 0, out, cap)
            if n < 0:
                _check(n)
            if n <= cap:
                return list(out[:n])
            cap = n

    def claim_requirements(self, sim):
        """NewNodeClaims[0]'s requirement record of `sim` (this rank must have run it)."""
        l = _cons_lib()
        out = (ctypes.c_uint32 * max(l.ks_cons_requirement_words(self._h), 1))()
        _check(l.ks_cons_claim_requirements(self._h, sim, out))
        return bytes(out)

    def _launch_names(self, ids):
        l = _cons_lib()
        return [l.ks_cons_instance_type_name(self._h, i).decode() for i in ids]

    def claim_launch(self, sim):
        """The launch list of simulation `sim`'s replace command after run(launch_lists=True), on the rank that ran
        it (ks_cons_claim_launch): (instance-type names in OrderByPrice order cut to 100, their prices, the number
        of options)."""
        its, prices = (ctypes.c_int32 * 100)(), (ctypes.c_double * 100)()
        n, nopt = ctypes.c_int(), ctypes.c_int()
        _check(_cons_lib().ks_cons_claim_launch(self._h, sim, its, prices, ctypes.byref(n), ctypes.byref(nopt)))
        return self._launch_names(its[:n.value]), list(prices[:n.value]), nopt.value

    def disrupt_launch(self, i):
        """The launch list of replacement `i` of the last disrupt(launch_lists=True) (ks_cons_disrupt_launch), as
        claim_launch returns it."""
        its, prices = ctypes.POINTER(ctypes.c_int32)(), ctypes.POINTER(ctypes.c_double)()
        n, nopt = ctypes.c_int(), ctypes.c_int()
        _check(_cons_lib().ks_cons_disrupt_launch(self._h, i, ctypes.byref(its), ctypes.byref(prices), ctypes.byref(n),
                                                  ctypes.byref(nopt)))
        return self._launch_names(its[:n.value]), list(prices[:n.value]), nopt.value

    def launch_ms(self):
        """HIP-event time of the launch-list kernel of the last run() / disrupt() (0 when none computed a list)."""
        return _cons_lib().ks_cons_launch_ms(self._h)

    def decide(self, records, world=1, all_sims=False, fetch=None, candidates=True, clock=None, sims=True):
        """Sequential selection over the gathered records ([rank][slot] layout, bytes).  fetch(sim)
        returns the requirement record bytes of a needed simulation (default: this handle's run);
        candidates=False leaves out the ordered candidate list and sims=False the per-simulation lists (the
        commands are unchanged);
        clock=(multi_timeout_s, single_timeout_s, sim_seconds): the methods' timeouts on a virtual clock."""
        l = _cons_lib()
        if fetch is None and world == 1:
            tbuf = None  # this handle ran every simulation: the library reads the requirement records it needs
        else:
            need = self.needed_sims(records, world, all_sims)
            fetch = fetch or self.claim_requirements
            table = b"".join(fetch(s) for s in need)
            tbuf = ctypes.create_string_buffer(table, max(len(table), 4))
        buf = None if records is None else _records_buffer(records)  # None: the handle's own records (run(keep=True))
        js = ctypes.c_void_p()
        flags = (1 if all_sims else 0) | (2 if candidates else 0) | (0 if sims else 4)
        if clock is None:
            _check(l.ks_cons_decide(self._h, ctypes.cast(buf, ctypes.c_void_p), world, flags,
                                    None if tbuf is None else ctypes.cast(tbuf, ctypes.c_void_p), ctypes.byref(js)))
        else:
            clk = _Clock(*clock)
            _check(l.ks_cons_decide_clock(self._h, ctypes.cast(buf, ctypes.c_void_p), world, flags,
                                          None if tbuf is None else ctypes.cast(tbuf, ctypes.c_void_p), ctypes.byref(clk),
                                          ctypes.byref(js)))
        return json.loads(_take_str(js))

    def validate(self, command, device=-1):
        """Validation.IsValid after its wait + ValidateCommand (validation.go:68-180): `command` (a
        decide() command, computed on an earlier snapshot) re-checked against this handle's snapshot,
        its re-simulation run on the GPU.  Returns {"valid", "reason", "sim"}."""
        b = (command if isinstance(command, str) else json.dumps(command)).encode()
        js = ctypes.c_void_p()
        o = _Opts(device, 1, 1, 0, 0)
        _check(_cons_lib().ks_cons_validate(self._h, b, len(b), ctypes.byref(o), ctypes.byref(js)))
        return json.loads(_take_str(js))

    def disrupt(self, method, all_sims=False, device=-1, lds_budget=0, launch_lists=False, placements=False):
        """Drift / Expiration ComputeCommand ("drift" | "expiration") on the handle's current state
        (ks_cons_disrupt): {"method", "candidates", "command": {"action", "candidates", "replacements"}, "sims",
        "plan", "kernel_ms"}.  The pass's plan and records survive the call.  launch_lists: every replacement also
        carries launchInstanceTypes / launchPrices (disrupt_launch reads them without JSON).  placements
        (KS_CONS_PLACEMENTS): a replace command's picked simulation runs once more with its commit log; every
        replacement gains "pods" (UIDs in commit order), its "requests" are rendered from the log (no refusal for
        mixed quantity formats), and the document gains "placements_ms"."""
        js = ctypes.c_void_p()
        o = _Opts(device, 1, 1, 0, lds_budget, 1 if launch_lists else 0)
        flags = (1 if all_sims else 0) | (KS_CONS_PLACEMENTS if placements else 0)
        _check(_cons_lib().ks_cons_disrupt(self._h, _method(method), ctypes.byref(o), flags, ctypes.byref(js)))
        return json.loads(_take_str(js))

    def sim_results(self, sim, device=-1, lds_budget=0):
        """Simulation Results of simulation `sim` of the last run() (ks_cons_sim_results): {"sim", "candidates",
        "allNonPendingScheduled", "newNodeClaims": [{nodePoolName, instanceTypeOptions, requests, requirements,
        pods}], "existingNodes": [{name, pods}], "unscheduled", "kernel_ms"}, pods as UIDs in commit order.  The
        simulation runs once more with its commit log; KsError (KS_ERR_ARG) before the first run, after update()
        until the next run, for another rank's simulation and for `sim` out of range."""
        js = ctypes.c_void_p()
        o = _Opts(device, 1, 1, 0, lds_budget, 0)
        _check(_cons_lib().ks_cons_sim_results(self._h, sim, ctypes.byref(o), ctypes.byref(js)))
        return json.loads(_take_str(js))

    def sim_counters(self, sim):
        """Solve counters of simulation `sim` from the last run (ks_problem.h Counter order)."""
        out = (ctypes.c_int64 * 64)()  # the library copies min(64, its counter count) and returns that count
        n = _cons_lib().ks_cons_sim_counters_n(self._h, sim, out, 64)
        if n < 0:
            _check(n)
        return list(out)[:n]

    def queue_readback(self):
        """Test / diagnostic read-back after run() (ks_cons_queue_readback): the queue inputs of the handle's pods
        (as queue_inputs) plus "n", "sims", "rbits", "sbits", and the arrays "lentries", "lentrySim", "lpodmap",
        "lrunlen" (n ints each) and "rank" (P ints) as they stand on the device."""
        import numpy as np

        meta, words, nw = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
        _check(_cons_lib().ks_cons_queue_readback(self._h, ctypes.byref(meta), ctypes.byref(words), ctypes.byref(nw)))
        try:
            arr = np.frombuffer(ctypes.string_at(words, nw.value * 4), dtype=np.int32).tolist()
        finally:
            lib().ks_free(words)
        doc = json.loads(_take_str(meta))
        n = doc["n"]
        assert len(arr) == 4 * n + doc["P"]
        for k, name in enumerate(("lentries", "lentrySim", "lpodmap", "lrunlen")):
            doc[name] = arr[k * n:(k + 1) * n]
        doc["rank"] = arr[4 * n:]
        return doc

    @property
    def last_reruns(self):
        """Multi-node probes the last decide() / needed_sims() re-simulated on this GPU from the pod objects
        earlier probes relaxed (ks_cons_last_reruns; -1: no decision yet)."""
        return _cons_lib().ks_cons_last_reruns(self._h)

    @property
    def last_routes(self):
        """The k_solve launches since the last run() began, in order (ks_cons_last_routes): a list of
        {"family", "rt", "tl", "lean", "n"[, "nmw"]}; re-runs of decide() and validate() append theirs."""
        js = ctypes.c_void_p()
        _check(_cons_lib().ks_cons_last_routes(self._h, ctypes.byref(js)))
        return json.loads(_take_str(js))

    def alg_bytes(self, records, world=1):
        if records is None:
            return _cons_lib().ks_cons_records_alg_bytes(self._h, None, world)
        buf = _records_buffer(records)
        return _cons_lib().ks_cons_records_alg_bytes(self._h, ctypes.cast(buf, ctypes.c_void_p), world)

    def consolidate(self, all_sims=False, device=-1, clock=None, launch_lists=False):
        recs, ms = self.run(0, 1, device, launch_lists=launch_lists)
        doc = self.decide(recs, 1, all_sims, clock=clock)
        doc["kernel_ms"] = ms
        return doc

    def close(self):
        if self._h:
            _cons_lib().ks_cons_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
