// bwd_record.hpp -- the record of one fused subtree of the backward sweep (solve_bwd_kernel_subtree, kernels_global.hpp; built by
// sweep_plan.hpp bwd_subtree_record) and its host check.  Plain C++: the device translation unit, the host's plan, tests/bwd_record_shim.cpp
// and tests/cpp/sweep_plan.cpp all read it.  The forward sweep's twin: fwd_record.hpp.
//
// The record (ints), copied to LDS once by the subtree's workgroup:
//   header of BS_HDR ints: the fields BS_LEVELS.. below -- the x area, the staged vectors and the end of the workgroup's LDS in doubles
//   from the start of LDS; then three lists of BS_LEVELS + 1 level pointers: into the members, into the tasks and into the stage table
//   (levels top-down, the subtree's root first); from BS_MEM0 the members, BS_MEM ints each (fields BS_K..); from BS_TASK0 the tasks,
//   one int each: member * 16 + four-column group; from BS_STAGE0 the stage table.
//   A member: k columns, r front rows beyond them, first node, BS_XOFF where its x is kept for its descendants (a double offset in the
//   x area; -1: no member below it reads it), BS_VOFF where [w_s; -x(R_s)] is staged while its level runs (a double offset in the
//   staging area), BS_ROW0 its first row in the stage table, the panel offset as two ints.
//   The stage table: one int per row of every member's staged vector, the members in order, so that row q of a level goes to double
//   offset 3 q of the staging area: e >= 0: -x from double offset e of the x area (the row's node is a column of a member at a higher
//   level of this subtree); e < 0, n = -1 - e: node n >> 1, from global W as it is (n odd: one of the member's own columns) or from
//   global X negated (n even: the node lies above the subtree).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "fwd_record.hpp"      // (sub_split64 / sub_join64: the panel offset's two ints)

namespace admm_dev {

constexpr int BS_LEVELS = 0, BS_NMEM = 1, BS_MEM0 = 2, BS_NTASK = 3, BS_TASK0 = 4, BS_XBUF = 5, BS_VBUF = 6, BS_END = 7, BS_NSTAGE = 8, BS_STAGE0 = 9, BS_HDR = 12;
constexpr int BS_K = 0, BS_R = 1, BS_FIRST = 2, BS_XOFF = 3, BS_VOFF = 4, BS_ROW0 = 5, BS_POFF = 6 /* two ints */, BS_MEM = BS_POFF + 2;
constexpr int64_t BS_MAX_NODES = (int64_t)1 << 29;      // (a stage entry holds 2 * node + 1)
constexpr int BS_KMAX = 64;      // columns of a member at most (16 four-column groups: a task's low four bits)

// Is `rec` (n_ints ints) a record the kernel may run?  Every offset inside its area, every member column written exactly once (by
// exactly one task, and into x slots no other member owns), every in-subtree row a column of a member at a higher level, every
// row from above the subtree outside every member.  n_nodes, panels_size: the extent of W / X (nodes) and of the panels (doubles).
// false: msg says what is wrong.
inline bool bwd_record_check(const int *rec, int64_t n_ints, int64_t n_nodes, int64_t panels_size, char *msg, int msg_len) {
    auto bad = [&](const char *what, long long a, long long b) { snprintf(msg, (size_t)msg_len, "backward subtree record: %s (%lld, %lld)", what, a, b); return false; };
    if (n_ints < BS_HDR || (n_ints & 3)) return bad("record size", n_ints, 0);
    const int64_t nl = rec[BS_LEVELS], nm = rec[BS_NMEM], m0 = rec[BS_MEM0], nt = rec[BS_NTASK], t0 = rec[BS_TASK0];
    const int64_t xb = rec[BS_XBUF], vb = rec[BS_VBUF], end = rec[BS_END], nst = rec[BS_NSTAGE], s0 = rec[BS_STAGE0];
    if (n_nodes > BS_MAX_NODES) return bad("too many nodes", n_nodes, 0);
    if (nl < 1 || nm < 1 || nt < 1 || nst < 1) return bad("empty", nl, nm);
    if (BS_HDR + 3 * (nl + 1) > m0 || m0 + BS_MEM * nm > t0 || t0 + nt > s0 || s0 + nst > n_ints) return bad("areas of the record overlap", m0, t0);
    if (2 * xb < n_ints || xb > vb || vb > end) return bad("LDS areas out of order", xb, vb);
    const int64_t xsize = vb - xb, vsize = end - vb;
    const int *lvm = rec + BS_HDR, *lvt = rec + BS_HDR + nl + 1, *lvs = rec + BS_HDR + 2 * (nl + 1);
    if (lvm[0] != 0 || lvm[nl] != nm || lvt[0] != 0 || lvt[nl] != nt || lvs[0] != 0 || lvs[nl] != nst) return bad("level pointers", lvm[nl], lvt[nl]);
    for (int64_t l = 0; l < nl; ++l) if (lvm[l] >= lvm[l + 1] || lvt[l] >= lvt[l + 1] || lvs[l] >= lvs[l + 1]) return bad("empty level", l, lvm[l]);
    for (int64_t l = 0; l < nl; ++l) if (3 * ((int64_t)lvs[l + 1] - lvs[l]) > vsize) return bad("staged level beyond the staging area", l, lvs[l + 1] - lvs[l]);
    std::vector<int> level_of(nm, -1);
    for (int64_t l = 0; l < nl; ++l) for (int q = lvm[l]; q < lvm[l + 1]; ++q) level_of[q] = (int)l;
    // members: extents, and who owns which slot of the x area (x_owner[e / 3] = member) and of a level's staging area
    std::vector<int> x_owner((size_t)(xsize / 3 + 1), -1);
    for (int64_t q = 0; q < nm; ++q) {
        const int *M = rec + m0 + BS_MEM * q;
        const int64_t k = M[BS_K], r = M[BS_R], first = M[BS_FIRST], xo = M[BS_XOFF], vo = M[BS_VOFF], r0 = M[BS_ROW0];
        const int64_t poff = sub_join64(M[BS_POFF], M[BS_POFF + 1]);
        if (k < 1 || k > BS_KMAX || r < 0) return bad("member shape", q, k);
        if (first < 0 || first + k > n_nodes) return bad("member columns outside the system", q, first);
        if (poff < 0 || poff + (k + r) * k > panels_size) return bad("panel offset", q, poff);
        if (vo < 0 || vo % 3 || vo + 3 * (k + r) > vsize) return bad("staging offset", q, vo);
        if (r0 < lvs[level_of[q]] || r0 + k + r > lvs[level_of[q] + 1]) return bad("stage rows outside the member's level", q, r0);
        if (vo != 3 * (r0 - lvs[level_of[q]])) return bad("staging offset is not the stage rows'", q, vo);
        if (xo < -1 || (xo >= 0 && (xo % 3 || xo + 3 * k > xsize))) return bad("x offset", q, xo);
        if (xo >= 0) for (int64_t j = 0; j < k; ++j) {
            if (x_owner[xo / 3 + j] >= 0) return bad("x slot written twice", q, x_owner[xo / 3 + j]);
            x_owner[xo / 3 + j] = (int)q;
        }
    }
    for (int64_t l = 0; l < nl; ++l) {      // ... and they fill the level's stage rows: no row of the table is left to chance
        int64_t rows = 0;
        for (int q = lvm[l]; q < lvm[l + 1]; ++q) rows += (int64_t)rec[m0 + BS_MEM * q + BS_K] + rec[m0 + BS_MEM * q + BS_R];
        if (rows != (int64_t)lvs[l + 1] - lvs[l]) return bad("stage rows of a level are not its members' rows", l, rows);
    }
    for (int64_t l = 0; l < nl; ++l)      // staged vectors of one level: disjoint
        for (int a = lvm[l]; a < lvm[l + 1]; ++a) for (int b = a + 1; b < lvm[l + 1]; ++b) {
            const int *A = rec + m0 + BS_MEM * a, *B = rec + m0 + BS_MEM * b;
            const int64_t a0 = A[BS_VOFF], a1 = a0 + 3 * ((int64_t)A[BS_K] + A[BS_R]), b0 = B[BS_VOFF], b1 = b0 + 3 * ((int64_t)B[BS_K] + B[BS_R]);
            if (a0 < b1 && b0 < a1) return bad("staged vectors overlap", a, b);
        }
    // tasks: inside their level, every four-column group of every member exactly once
    std::vector<int> seen((size_t)nm * 16, 0);
    for (int64_t l = 0; l < nl; ++l) for (int t = lvt[l]; t < lvt[l + 1]; ++t) {
        const int v = rec[t0 + t], q = v >> 4, g = v & 15;
        if (v < 0 || q >= nm) return bad("task member", t, q);
        if (level_of[q] != l) return bad("task outside its member's level", t, q);
        if (4 * g >= rec[m0 + BS_MEM * q + BS_K]) return bad("task beyond the member's columns", t, g);
        if (seen[(size_t)q * 16 + g]++) return bad("column written twice", q, 4 * g);
    }
    for (int64_t q = 0; q < nm; ++q) for (int g = 0; 4 * g < rec[m0 + BS_MEM * q + BS_K]; ++g)
        if (!seen[(size_t)q * 16 + g]) return bad("column never written", q, 4 * g);
    // the stage table: a member's own columns from W, then its front rows
    for (int64_t q = 0; q < nm; ++q) {
        const int *M = rec + m0 + BS_MEM * q;
        const int *st = rec + s0 + M[BS_ROW0];
        for (int i = 0; i < M[BS_K] + M[BS_R]; ++i) {
            const int64_t e = st[i];
            if (i < M[BS_K]) {
                if (e != -1 - (2 * ((int64_t)M[BS_FIRST] + i) + 1)) return bad("own column not staged from w", q, i);
            } else if (e >= 0) {
                if (e % 3 || e + 3 > xsize || x_owner[e / 3] < 0) return bad("row outside the x area", q, e);
                if (level_of[x_owner[e / 3]] >= level_of[q]) return bad("row of a member that is not at a higher level", q, x_owner[e / 3]);
            } else {
                const int64_t n = -1 - e, node = n >> 1;
                if (n & 1) return bad("front row staged from w", q, i);
                if (node >= n_nodes) return bad("row outside the system", q, node);
                for (int64_t p = 0; p < nm; ++p) {
                    const int *P = rec + m0 + BS_MEM * p;
                    if (node >= P[BS_FIRST] && node < (int64_t)P[BS_FIRST] + P[BS_K]) return bad("row read from global x lies inside the subtree", q, node);
                }
            }
        }
    }
    return true;
}

}   // namespace admm_dev
