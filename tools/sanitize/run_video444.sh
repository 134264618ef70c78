#!/bin/bash
# The 4:4:4 packed-video kernels (kernels_video444.hip) compiled for the host with hip_shim/ in place of the HIP headers, built
# with -fsanitize=address,undefined into a stand-alone program and run over the cases video444_cases.py makes with the numpy
# statement: every format and container, the shapes and the three layouts (tight, pitched with a shifting alignment, pitched by
# a multiple of 256) of tests/test_gpu_video444.py.  CPU only.      tools/sanitize/run_video444.sh
set -e -o pipefail
ROOT="$(cd "$(dirname "$0")/../.." && pwd)"
W=/tmp/ojph_sanitize_video444; mkdir -p $W
g++ -std=c++17 -O1 -g -x c++ -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/tools/sanitize/hip_shim \
    $ROOT/tools/sanitize/video444_host.cpp -o $W/video444_host
python $ROOT/tools/sanitize/video444_cases.py $W/cases.bin
ASAN_OPTIONS=detect_leaks=1 UBSAN_OPTIONS=print_stacktrace=1 $W/video444_host $W/cases.bin 2>&1 | tail -25
