#!/bin/bash
# The rounds of the byte-budget search (ojphgpu_rate_rounds_*, openjph_amd/csrc/ojph_rate.cpp) with the plan builder they
# read, compiled for the host with -fsanitize=address,undefined into a stand-alone program (rate_rounds_host.cpp) and driven
# through searches of one and of four frames over synthetic monotone size tables.  CPU only.   tools/sanitize/run_rate_rounds.sh
set -e -o pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
W=/tmp/ojph_sanitize_rate_rounds; mkdir -p $W
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread \
    $ROOT/tools/sanitize/rate_rounds_host.cpp $ROOT/openjph_amd/csrc/ojph_rate.cpp $ROOT/openjph_amd/csrc/ojph_plan.cpp \
    $ROOT/openjph_amd/csrc/ojph_pool.cpp -o $W/rate_rounds_host
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 $W/rate_rounds_host 2>&1 | tail -25
