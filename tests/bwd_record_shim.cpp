// The host check of a fused backward subtree record (csrc/bwd_record.hpp bwd_record_check), compiled for the host so that
// tests/test_sweep_subtree_bwd.py can hand it records without a GPU: the very same header is what sweep_plan.hpp calls on every
// record it builds.
#include "../admm-elastic-sca_amd/csrc/bwd_record.hpp"

extern "C" {

// 1: the record may run; 0: refused, msg says why
int br_check(const int *rec, long long n_ints, long long n_nodes, long long panels_size, char *msg, int msg_len) {
    return admm_dev::bwd_record_check(rec, n_ints, n_nodes, panels_size, msg, msg_len) ? 1 : 0;
}

// the layout constants the test builds its record from
int br_const(int which) {
    using namespace admm_dev;
    const int v[] = {BS_LEVELS, BS_NMEM, BS_MEM0, BS_NTASK, BS_TASK0, BS_XBUF, BS_VBUF, BS_END, BS_NSTAGE, BS_STAGE0, BS_HDR,
                     BS_K, BS_R, BS_FIRST, BS_XOFF, BS_VOFF, BS_ROW0, BS_POFF, BS_MEM};
    return which >= 0 && which < (int)(sizeof v / sizeof v[0]) ? v[which] : -1;
}

}
