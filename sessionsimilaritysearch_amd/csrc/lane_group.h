// What the row kernels share around "one group of LPR lanes per row" (rowops.hip, gnn.hip, gnn_fused.hip, variants.hip,
// hgt.hip, text.hip, bert.hip): the lane-count rule, its switch to a template parameter, the grid rule, the butterfly
// inside a lane group, and the argument checks of rows that are read 16 bytes per lane.
#pragma once
#include <limits.h>

#include "sss_common.h"

namespace sss {

// Sum over the LPR lanes of a group (LPR a power of two, groups aligned inside the wave); every lane ends with the same bits.
template <int LPR, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Lanes per row of `width` floats: the smallest power of two that covers width / 4 float4 columns, a wave at the most
// (wider rows are walked in column chunks).  oracle/encoder_kernels_ref.py: lanes_for mirrors it for the tests' case tables.
static inline int lanes_for(int width) {
    const int nv = width / 4;
    int l = 1;
    while (l < nv && l < 64) l <<= 1;
    return l;
}

// Runs CALL with `constexpr int L = lpr` (lpr as lanes_for gives it).
#define SSS_LPR_SWITCH(lpr, CALL)                       \
    switch (lpr) {                                      \
        case 1: { constexpr int L = 1; CALL; } break;   \
        case 2: { constexpr int L = 2; CALL; } break;   \
        case 4: { constexpr int L = 4; CALL; } break;   \
        case 8: { constexpr int L = 8; CALL; } break;   \
        case 16: { constexpr int L = 16; CALL; } break; \
        case 32: { constexpr int L = 32; CALL; } break; \
        default: { constexpr int L = 64; CALL; } break; \
    }

// Workgroups for `items` rows (or elements) at `per_block` a workgroup, `cap` at the most.  A cap is only for a kernel
// that grid-strides over what is left; a kernel that gives every group exactly one row takes GRID_ALL, or rows are dropped.
constexpr long GRID_ALL = LONG_MAX;
static inline unsigned grid_blocks(long items, long per_block, long cap) {
    long g = (items + per_block - 1) / per_block;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

// the argument checks of rows read as float4 columns
static inline bool aligned16(const void* p) { return p && (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool ok_ld(int64_t ld, int width) { return ld % 4 == 0 && ld >= width; }
static inline bool ok_count(int64_t n) { return n >= 0 && n < (1ll << 31); }

}  // namespace sss
