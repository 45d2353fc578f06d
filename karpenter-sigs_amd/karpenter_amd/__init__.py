"""MI355X-native Karpenter scheduler hot path (Scheduler.Solve) — Python mirror of the C-ABI.

The product is libkarpenter_amd.so (HIP kernels for gfx950 + C-ABI, include/karpenter_amd.h).
This package only marshals snapshots and results; there is no CPU fallback: every entry point
raises if the HIP library is missing or no GPU is visible.
"""
from .scheduler import Consolidator, claim_sort_probe, claim_sort_probe_append, snapshot_check, encode_binary, check_binary, cluster_state, inspect_consolidation, inspect_consolidation_update, inspect_disruption, inspect_disruption_binary, encode_consolidation_binary, shard_slot, KsError, Results, Scheduler, StaticFeasibility, inspect, inspect_binary, lib, library_path, queue_inputs, rec_headers_meta, rec_headers_run, rec_headers_verdicts  # noqa: F401
