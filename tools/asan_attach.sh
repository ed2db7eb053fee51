#!/bin/bash
# CPU only: the host side of rigid attachments (csrc/attach_host.cpp, and the registration calls on a host-only context) under
# AddressSanitizer + UBSan in a stand-alone program of its own (tools/asan_attach.cpp) -- nothing is loaded into Python, no preloaded
# runtime.  The query is compiled into the program with the sanitizers; the context calls go into the library as built.
cd "$(dirname "$0")/.."
P=admm-elastic-sca_amd; B=tests/_build/asan_attach; mkdir -p $B
python3 -c "import __graft_entry__ as g; g.load_package().build()" > /dev/null || exit 1
g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -ffp-contract=off -Wno-unknown-pragmas -Iinclude \
    tools/asan_attach.cpp $P/csrc/attach_host.cpp -o $B/asan_attach -L$P -ladmm_hip -Wl,-rpath,$PWD/$P -Wl,-rpath,/opt/rocm/lib || exit 1
ASAN_OPTIONS=detect_leaks=0:halt_on_error=1 UBSAN_OPTIONS=print_stacktrace=1:halt_on_error=1 $B/asan_attach
rc=$?
rm -rf $B
exit $rc
