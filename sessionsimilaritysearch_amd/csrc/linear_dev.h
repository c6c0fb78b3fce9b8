// What the grouped GEMMs share (k_linear_grouped of linear.hip, k_linear_grouped_bf16 of linear_bf16.hip): the kernel
// argument and the epilogue of one accumulator element -- bias, activation, the optional scale / shift / relu stage and the
// store.  Both kernels run this one float32 arithmetic.
#pragma once
#include "sss_common.h"

namespace sss {

// The kernel's argument: the callers' problems as they are (sss_linear_problem, include/sss.h), each followed by what the
// launcher adds.  A slot is 128 bytes, so the scalar loads of a problem's fields stay aligned: four bare 120-byte problems
// with the launcher's tables behind or before them measured 1 - 2 % slower on every shape, 3 - 4 % on the smallest.
struct LinSlot {
    sss_linear_problem p;
    int tiles_m, tile_begin;           // filled by the launcher: the problem's column tiles, its first workgroup
};
static_assert(sizeof(LinSlot) == 128, "k_linear_grouped: one problem per 128 bytes of kernel argument");
struct LinBatch { LinSlot s[4]; int nprob, K; };

// One accumulator element `a` of output (row, col), col < M (the caller checks): bias, activation and the optional post
// stage, then the store when the row exists.  bv / ps / pt: the column's bias, post scale and post shift (ps and pt are
// read only when post_s).
__device__ __forceinline__ void linear_epilogue(float a, float bv, int act, const float* post_s, float ps, float pt, long row, long N,
                                                float* Y, long ldy, int col) {
    float v = a + bv;
    if (act == 1) v = fmaxf(v, 0.f);
    else if (act == 2) v = tanhf(v);
    else if (act == 3) v = v > 0.f ? 1.f : v < 0.f ? -1.f : v;     // torch.sign (0 and NaN pass through)
    else if (act == 4) v = tanhf(tanhf(v));
    else if (act == 5) v = gelu_erf(v);                             // exact GELU: gelu(0) = 0, NaN passes through
    if (post_s) {
#pragma clang fp contract(off)                                       // multiply, round, add, round: no fused fma here
        v = fmaxf(v * ps + pt, 0.f);                                // bn(x) in eval mode as scale / shift, then relu
    }
    if (row < N) Y[row * ldy + col] = v;
}

}  // namespace sss
