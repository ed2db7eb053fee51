// fwd_record.hpp -- the record of one fused subtree of the forward sweep (solve_fwd_subtree_kernel, kernels_global.hpp; built by
// sweep_plan.hpp plan_fused_subtrees) and the shape constants of the wave-per-tile forward kernels the plan reads.  Plain C++: the
// device translation unit, the host's plan and tests/cpp/sweep_plan.cpp all read it.  The twin of bwd_record.hpp.
//
// The record (ints), copied to LDS once by the subtree's workgroup: a header of SUB_HDR ints -- the fields SUB_LEVELS.. below, the
// contribution area and the staged vectors in doubles from the start of LDS -- then from SUB_HDR the level pointers (levels bottom-up),
// then items of SUB_ITEM ints (fields SUB_K..; the front map is an int offset in the record, -1 = no children; the destination of the
// contribution a double offset in the contribution area, -1 = C).
// A front map holds four ints per front row: double offsets of the children's rows in the contribution area.
#pragma once
#include <stdint.h>

#ifndef ADMM_HD                // (the same definition as local_math.hpp's)
#ifdef __HIPCC__
#define ADMM_HD __host__ __device__ __forceinline__
#else
#define ADMM_HD inline
#endif
#endif

namespace admm_dev {

constexpr int FWD_SMALL_KMAX = 64;    // columns of a supernode at most in the wave-per-tile forward kernels
constexpr int FWD_SMALL_WAVES = 4;    // wave items per block in the narrow-supernode forward kernel

constexpr int SUB_LEVELS = 0, SUB_ITEM0 = 1, SUB_CBUF = 2, SUB_TS = 3, SUB_ROOT_SLOT = 4 /* two ints */, SUB_HDR = 8;
constexpr int SUB_K = 0, SUB_R = 1, SUB_FIRST = 2, SUB_TILE = 3, SUB_MAP = 4, SUB_CDST = 5, SUB_POFF = 6 /* two ints */, SUB_ITEM = SUB_POFF + 2;
constexpr int SUB_WAVES = 8;      // waves per subtree workgroup
// 64-bit record fields as (low, high) int pairs
ADMM_HD void sub_split64(int64_t v, int *lohi) { lohi[0] = (int)(uint32_t)(v & 0xffffffff); lohi[1] = (int)(v >> 32); }
ADMM_HD int64_t sub_join64(int lo, int hi) { return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo); }

}   // namespace admm_dev
