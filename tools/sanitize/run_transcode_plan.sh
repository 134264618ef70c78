#!/bin/bash
# The output plan of a transcode (ojphgpu_plan_create_transcode, openjph_amd/csrc/ojph_transcode.cpp) with the plan builder and
# the Tier-2 writer / parser it rests on, compiled for the host with -fsanitize=address,undefined into a stand-alone program
# (transcode_plan_host.cpp): sources written and parsed, the plan asked for with everything that may change and with every
# other field disturbed.  CPU only.   tools/sanitize/run_transcode_plan.sh
set -e -o pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
W=/tmp/ojph_sanitize_transcode_plan; mkdir -p $W
g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -pthread \
    -I$ROOT/include -I$ROOT/openjph_amd/csrc $ROOT/tools/sanitize/transcode_plan_host.cpp $ROOT/openjph_amd/csrc/ojph_transcode.cpp \
    $ROOT/openjph_amd/csrc/ojph_plan.cpp $ROOT/openjph_amd/csrc/ojph_t2.cpp $ROOT/openjph_amd/csrc/ojph_pool.cpp \
    $ROOT/openjph_amd/csrc/ht_tables.cpp -o $W/transcode_plan_host
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 $W/transcode_plan_host 2>&1 | tail -25
