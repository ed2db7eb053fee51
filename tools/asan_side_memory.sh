#!/bin/bash
# CPU only: the host routines of side memory (csrc/mesh.cpp) under AddressSanitizer + UBSan in a stand-alone program of their own
# (tools/asan_side_memory.cpp) -- nothing is loaded into Python, no preloaded runtime.
cd "$(dirname "$0")/.."
B=tests/_build/asan_side; mkdir -p $B
g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -fopenmp -ffp-contract=off -Wno-unknown-pragmas \
    tools/asan_side_memory.cpp admm-elastic-sca_amd/csrc/mesh.cpp -o $B/asan_side_memory || exit 1
ASAN_OPTIONS=detect_leaks=1:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $B/asan_side_memory
rc=$?
rm -rf $B
exit $rc
