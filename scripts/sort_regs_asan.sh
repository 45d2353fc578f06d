#!/bin/bash
# AddressSanitizer + UndefinedBehaviorSanitizer over the lane model of the register-copy claim re-sort
# (csrc/ks_sort_regs.h with csrc/ks_gosort.h), in a stand-alone program of its own (scripts/sort_regs_host_main.cpp):
# host code only, no device, nothing loaded into an interpreter.  Any report aborts the run.
set -euo pipefail
cd "$(dirname "$0")/.."
out=$(mktemp -d)
trap 'rm -rf "$out"' EXIT
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined \
  scripts/sort_regs_host_main.cpp -o "$out/run"
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=halt_on_error=1:print_stacktrace=1 "$out/run"
