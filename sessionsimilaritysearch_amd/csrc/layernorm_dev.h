// The row statistics and the store of the wave-per-row LayerNorm kernels (k_add_layernorm in text.hip, k_bert_embed in
// bert.hip): one wave owns a row, a lane holds the float4 columns lane, lane + 64, ... (at most 4: e <= 1024).
#pragma once
#include "sss_common.h"

namespace sss {

// The lane's share of the row's sum, in the order every caller adds it up.
__device__ __forceinline__ float ln_lane_sum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }

// v holds the lane's columns of the row (zeros where (lane + 64 j) * 4 >= e) and `sum` the lane's share of their sum.
// Two passes: the mean, then the sum of squared deviations from it (biased variance) plus eps -- never E[x^2] - E[x]^2.
// Writes yrow[:e] = (v - mean) * rstd * gamma + beta and yrow[e:ld_y] = 0.  The whole wave must call it (shuffles).
__device__ __forceinline__ void ln_row_store(float4 (&v)[4], float sum, const float* __restrict__ gamma, const float* __restrict__ beta,
                                             float eps, int e, int lane, float* yrow, long ld_y) {
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)e;
    float sq = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if ((lane + 64 * j) * 4 < e) {
            v[j].x -= mean; v[j].y -= mean; v[j].z -= mean; v[j].w -= mean;
            sq += (v[j].x * v[j].x + v[j].y * v[j].y) + (v[j].z * v[j].z + v[j].w * v[j].w);
        }
    }
    for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
    const float rstd = 1.f / sqrtf(sq / (float)e + eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (lane + 64 * j) * 4;
        if (c < e) {
            const float4 g = *reinterpret_cast<const float4*>(gamma + c);
            const float4 b = *reinterpret_cast<const float4*>(beta + c);
            *reinterpret_cast<float4*>(yrow + c) = make_float4(v[j].x * rstd * g.x + b.x, v[j].y * rstd * g.y + b.y,
                                                               v[j].z * rstd * g.z + b.z, v[j].w * rstd * g.w + b.w);
        }
    }
    for (int c = e + lane * 4; c < ld_y; c += 256) *reinterpret_cast<float4*>(yrow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
}

}  // namespace sss
