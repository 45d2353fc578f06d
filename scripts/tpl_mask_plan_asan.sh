#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the LEAN Solve's mask-table arithmetic (csrc/ks_tplmask.h) and a
# replay of the kernel's row stores on a buffer of the planned size, in a stand-alone program of its own
# (scripts/tpl_mask_plan_main.cpp): host code only, no device, nothing loaded into an interpreter.  Any report
# aborts the run.
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  scripts/tpl_mask_plan_main.cpp -o "$out/run"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$out/run"
