// The embedding stage of the node text encoder (gfx950; include/sss_bert.h states the computation, DESIGN.md section 5.10
// derives it from BertEmbeddings.forward) on packed token rows:
//   k_bert_embed      x = LayerNorm((word[tok] + type[tt]) + pos[p]) * gamma + beta, pad columns zeroed
// One wave per row, four rows per workgroup, a lane holds the float4 columns lane, lane + 64, ... -- the lane map of
// k_add_layernorm (text.hip), with which it shares the row statistics and the store (layernorm_dev.h).  The rest of a BERT
// layer is k_linear_grouped (linear.hip; act = 5 is the exact GELU), k_seq_attention and k_add_layernorm (text.hip).
#include "lane_group.h"
#include "layernorm_dev.h"
#include "../../include/sss_bert.h"

namespace sss {

__global__ __launch_bounds__(256) void k_bert_embed(const float* __restrict__ word, long n_word, const float* __restrict__ type, long n_type,
                                                    const float* __restrict__ pos, long n_pos, const long* __restrict__ tok,
                                                    const int* __restrict__ tt, const int* __restrict__ p,
                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps, long n,
                                                    int e, float* __restrict__ x, long ld_x, int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;                                       // a whole wave leaves: the shuffles below stay convergent
    const long t = tok[r], ty = tt[r], ps = p[r];             // one row per wave: the branch below is wave-uniform
    float* xrow = x + r * ld_x;
    if (t < 0 || t >= n_word || ty < 0 || ty >= n_type || ps < 0 || ps >= n_pos) {
        for (int c = lane * 4; c < ld_x; c += 256) *reinterpret_cast<float4*>(xrow + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane == 0) *err = 1;
        return;
    }
    float4 v[4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (lane + 64 * j) * 4;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < e) {
            const float4 a = *reinterpret_cast<const float4*>(word + t * e + c);
            const float4 b = *reinterpret_cast<const float4*>(type + ty * e + c);
            const float4 d = *reinterpret_cast<const float4*>(pos + ps * e + c);
            v[j] = make_float4((a.x + b.x) + d.x, (a.y + b.y) + d.y, (a.z + b.z) + d.z, (a.w + b.w) + d.w);
            sum += ln_lane_sum(v[j]);
        }
    }
    ln_row_store(v, sum, gamma, beta, eps, e, lane, xrow, ld_x);
}

extern "C" int sss_bert_embed(const float* word, int64_t n_word, const float* type, int64_t n_type, const float* pos, int64_t n_pos,
                              const int64_t* tok, const int32_t* tt, const int32_t* p, const float* gamma, const float* beta, float eps,
                              int64_t n, int e, float* x, int64_t ld_x, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e < 4 || e % 4 || e > 1024 || !ok_ld(ld_x, e)) { set_error("bert_embed: need e %% 4 == 0, 4 <= e <= 1024, ld_x %% 4 == 0 and >= e"); return SSS_EINVAL; }
    if (n_word < 1 || n_type < 1 || n_pos < 1 || !(eps > 0.f) || !ok_count(n)) {
        set_error("bert_embed: need n_word, n_type, n_pos >= 1, eps > 0 and 0 <= n < 2^31");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    if (!aligned16(word) || !aligned16(type) || !aligned16(pos) || !aligned16(gamma) || !aligned16(beta) || !aligned16(x) || !tok || !tt ||
        !p || !err) {
        set_error("bert_embed: need non-null 16-byte aligned word / type / pos / gamma / beta / x and non-null tok / tt / p / err");
        return SSS_EINVAL;
    }
    hipLaunchKernelGGL(k_bert_embed, dim3(grid_blocks(n, 4, GRID_ALL)), dim3(256), 0, st, word, (long)n_word, type, (long)n_type, pos,
                       (long)n_pos, reinterpret_cast<const long*>(tok), tt, p, gamma, beta, eps, (long)n, e, x, (long)ld_x, err);
    return check_launch("k_bert_embed");
}

}  // namespace sss
