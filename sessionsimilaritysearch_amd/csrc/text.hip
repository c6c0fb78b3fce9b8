// The row kernels of the query text encoder (gfx950; include/sss_text.h states each computation, DESIGN.md section 5.9
// derives them from the reference's NodeTextTransformer, model/NodeEmbedding.py:62-98) on packed token rows.  The GEMMs of
// a layer are k_linear_grouped (linear.hip); these three are what is left between them:
//   k_text_embed      x = table[tok] * sqrt(e) + pe[pos], two roundings, pad columns zeroed
//   k_seq_attention   multi-head softmax attention inside each packed sequence of at most 64 rows
//   k_add_layernorm   y = LayerNorm(x + res) * gamma + beta, two-pass variance, in place allowed
// Lane map of k_seq_attention: one wave per (sequence, head).  The head's K and V rows are staged in LDS with a row stride
// of DC floats (DC = 32 or 64, the head-width ceiling; columns [D, DC) are zeros, so the inner loops carry no predicate) and
// lane t owns query row t, with q and the output accumulator in registers: every ds_read_b128 of the key loop has one
// address for the whole wave, a broadcast.  Q goes in, and the result comes out, through a third LDS tile of row stride
// DC + 1 (lane t reads / writes its own row: DC + 1 is odd, so the 32 lanes of a half wave hit 32 different banks) so
// that both global accesses walk rows with consecutive lanes on consecutive columns.  One pass over the keys (online
// softmax, the idiom of k_hgt_aggregate).  At T = 20 a wave has 20 of 64 lanes at work; see DESIGN.md 5.9.
#include <math.h>

#include "lane_group.h"
#include "layernorm_dev.h"
#include "../../include/sss_text.h"

namespace sss {

__global__ __launch_bounds__(256) void k_text_embed(const float* __restrict__ table, long n_token, const float* __restrict__ pe,
                                                    long n_pos, const long* __restrict__ tok, const int* __restrict__ pos, long n,
                                                    int e, float scale, float* __restrict__ x, long ld_x, int* __restrict__ err) {
    const int ld4 = (int)(ld_x / 4);
    const long total = n * ld4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / ld4;
        const int c = (int)(idx % ld4) * 4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < e) {
            const long t = tok[r];
            const long p = pos[r];
            if (t >= 0 && t < n_token && p >= 0 && p < n_pos) {
                const float4 a = *reinterpret_cast<const float4*>(table + t * e + c);
                const float4 b = *reinterpret_cast<const float4*>(pe + p * e + c);
                // a product rounded to float32, then a sum rounded to float32: what torch computes (hipcc contracts
                // a * b + c into one fma by default, and HIP's __fmul_rn / __fadd_rn are plain operators, no barrier)
                {
#pragma clang fp contract(off)
                    o.x = a.x * scale + b.x; o.y = a.y * scale + b.y; o.z = a.z * scale + b.z; o.w = a.w * scale + b.w;
                }
            } else if (c == 0) {
                *err = 1;
            }
        }
        *reinterpret_cast<float4*>(x + r * ld_x + c) = o;
    }
}

// floats of LDS one wave of k_seq_attention takes: K and V tiles [L, DC], the Q / result tile [L, DC + 1] rounded up so
// that the next wave's K tile stays 16-byte aligned
static __host__ __device__ inline int attn_wave_floats(int L, int DC) { return 2 * L * DC + (L * (DC + 1) + 3) / 4 * 4; }

template <int DC>
__global__ __launch_bounds__(256) void k_seq_attention(const sss_seq_attention_args A) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = A.max_len, D = A.head_dim, e = A.heads * D;
    float* Ks = lds + (long)wave * attn_wave_floats(L, DC);
    float* Vs = Ks + L * DC;
    float* Qs = Vs + L * DC;                                  // row stride DC + 1
    const long item = (long)blockIdx.x * (blockDim.x >> 6) + wave;
    long r0 = 0;
    int len = 0, hoff = 0;
    if (item < A.n_seq * A.heads) {                           // no early return: the barriers below stay convergent
        const long s = item / A.heads;
        hoff = (int)(item % A.heads) * D;
        const long a = A.ptr[s], b = A.ptr[s + 1];
        r0 = a < 0 ? 0 : (a > A.n_rows ? A.n_rows : a);       // whatever ptr holds, rows [r0, r0 + len) exist
        const long r1 = b > A.n_rows ? A.n_rows : b;
        len = r1 - r0 > L ? L : (r1 > r0 ? (int)(r1 - r0) : 0);
    }
    for (int idx = lane; idx < len * DC; idx += 64) {
        const int j = idx / DC, d = idx % DC;
        float q = 0.f, k = 0.f, v = 0.f;
        if (d < D) {
            const float* p = A.qkv + (r0 + j) * A.ld_qkv + hoff + d;
            q = p[0]; k = p[e]; v = p[2 * e];
        }
        Ks[j * DC + d] = k;
        Vs[j * DC + d] = v;
        Qs[j * (DC + 1) + d] = q;
    }
    const unsigned long long keys = __ballot(lane < len && A.key_ok[r0 + lane] != 0);
    __syncthreads();
    if (lane < len) {
        float q[DC], acc[DC];
#pragma unroll
        for (int d = 0; d < DC; ++d) { q[d] = Qs[lane * (DC + 1) + d]; acc[d] = 0.f; }
        float mx = -INFINITY, den = 0.f;
        for (int j = 0; j < len; ++j) {
            if (!((keys >> j) & 1)) continue;                 // wave-uniform
            const float4* kr = reinterpret_cast<const float4*>(Ks + j * DC);
            float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;     // four chains, always summed in this order
#pragma unroll
            for (int d = 0; d < DC / 4; ++d) {
                const float4 kk = kr[d];
                p0 += q[4 * d] * kk.x; p1 += q[4 * d + 1] * kk.y; p2 += q[4 * d + 2] * kk.z; p3 += q[4 * d + 3] * kk.w;
            }
            const float sc = (p0 + p1) + (p2 + p3);
            if (sc > mx) {
                const float f = expf(mx - sc);                // exp(-inf) = 0 on the first key
                den *= f;
#pragma unroll
                for (int d = 0; d < DC; ++d) acc[d] *= f;
                mx = sc;
            }
            const float ex = expf(sc - mx);
            den += ex;
            const float4* vr = reinterpret_cast<const float4*>(Vs + j * DC);
#pragma unroll
            for (int d = 0; d < DC / 4; ++d) {
                const float4 vv = vr[d];
                acc[4 * d] += ex * vv.x; acc[4 * d + 1] += ex * vv.y; acc[4 * d + 2] += ex * vv.z; acc[4 * d + 3] += ex * vv.w;
            }
        }
        const float inv = den > 0.f ? 1.f / den : 0.f;        // no valid key: zeros, never NaN
#pragma unroll
        for (int d = 0; d < DC; ++d) Qs[lane * (DC + 1) + d] = acc[d] * inv;
    }
    __syncthreads();
    for (int idx = lane; idx < len * DC; idx += 64) {
        const int j = idx / DC, d = idx % DC;
        if (d < D) A.out[(r0 + j) * A.ld_out + hoff + d] = Qs[j * (DC + 1) + d];
    }
    if (hoff == 0) {                                          // head 0 also zeroes the row's pad columns
        const int pad = (int)(A.ld_out - e);
        for (int idx = lane; idx < len * pad; idx += 64) A.out[(r0 + idx / pad) * A.ld_out + e + idx % pad] = 0.f;
    }
}

// One wave per row, four rows per workgroup; a lane holds the float4 columns lane, lane + 64, ... (at most 4: e <= 1024).
__global__ __launch_bounds__(256) void k_add_layernorm(const float* x, long ld_x, const float* res, long ld_res,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                       long n, int e, float* y, long ld_y) {
    const int lane = threadIdx.x & 63;
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;                                       // a whole wave leaves: the shuffles below stay convergent
    float4 v[4];
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (lane + 64 * j) * 4;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < e) {
            const float4 a = *reinterpret_cast<const float4*>(x + r * ld_x + c);
            const float4 b = *reinterpret_cast<const float4*>(res + r * ld_res + c);
            v[j] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
            sum += ln_lane_sum(v[j]);
        }
    }
    ln_row_store(v, sum, gamma, beta, eps, e, lane, y + r * ld_y, ld_y);   // layernorm_dev.h: shared with k_bert_embed
}

extern "C" int sss_text_embed(const float* table, int64_t n_token, const float* pe, int64_t n_pos, const int64_t* tok,
                              const int32_t* pos, int64_t n, int e, float scale, float* x, int64_t ld_x, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e < 4 || e % 4 || e > 1024 || !ok_ld(ld_x, e)) { set_error("text_embed: need e %% 4 == 0, 4 <= e <= 1024, ld_x %% 4 == 0 and >= e"); return SSS_EINVAL; }
    if (n_token < 1 || n_pos < 1 || !ok_count(n)) { set_error("text_embed: need n_token >= 1, n_pos >= 1 and 0 <= n < 2^31"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    if (!aligned16(table) || !aligned16(pe) || !aligned16(x) || !tok || !pos || !err) {
        set_error("text_embed: need non-null 16-byte aligned table / pe / x and non-null tok / pos / err");
        return SSS_EINVAL;
    }
    hipLaunchKernelGGL(k_text_embed, dim3(grid_blocks(n * (ld_x / 4), 256, 1 << 20)), dim3(256), 0, st, table, (long)n_token, pe,
                       (long)n_pos, reinterpret_cast<const long*>(tok), pos, (long)n, e, scale, x, (long)ld_x, err);
    return check_launch("k_text_embed");
}

extern "C" int sss_seq_attention(const sss_seq_attention_args* args, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!args) { set_error("seq_attention: null args"); return SSS_EINVAL; }
    const sss_seq_attention_args a = *args;
    if (a.head_dim < 1 || a.head_dim > 64 || a.heads < 1 || (long)a.heads * a.head_dim > 1024) {
        set_error("seq_attention: need 1 <= head_dim <= 64 and heads * head_dim <= 1024; got %d x %d", a.heads, a.head_dim);
        return SSS_EINVAL;
    }
    if (a.max_len < 1 || a.max_len > 64) { set_error("seq_attention: need 1 <= max_len <= 64, got %d", a.max_len); return SSS_EINVAL; }
    if (!ok_count(a.n_seq) || !ok_count(a.n_rows)) { set_error("seq_attention: need 0 <= n_seq, n_rows < 2^31"); return SSS_EINVAL; }
    const int e = a.heads * a.head_dim;
    if (a.ld_qkv < 3 * (int64_t)e || a.ld_out < e) { set_error("seq_attention: need ld_qkv >= 3 * heads * head_dim and ld_out >= heads * head_dim"); return SSS_EINVAL; }
    if (a.n_seq == 0 || a.n_rows == 0) return SSS_OK;
    if (!a.qkv || !a.out || !a.ptr || !a.key_ok || (reinterpret_cast<uintptr_t>(a.qkv) & 3) || (reinterpret_cast<uintptr_t>(a.out) & 3)) {
        set_error("seq_attention: need non-null qkv / ptr / key_ok / out, qkv and out 4-byte aligned");
        return SSS_EINVAL;
    }
    const long items = (long)a.n_seq * a.heads;
    const int dc = a.head_dim <= 32 ? 32 : 64;
    const size_t per_wave = (size_t)attn_wave_floats(a.max_len, dc) * sizeof(float);      // at most 49408 bytes
    int wpb = (int)(65536 / per_wave);                        // stay inside the 64 KiB every kernel may ask for
    wpb = wpb > 4 ? 4 : wpb;
    const long blocks = (items + wpb - 1) / wpb;
    if (blocks >= (1ll << 31)) { set_error("seq_attention: n_seq * heads = %ld is more than one launch takes", items); return SSS_EINVAL; }
    if (dc == 32) hipLaunchKernelGGL(k_seq_attention<32>, dim3((unsigned)blocks), dim3(64 * wpb), wpb * per_wave, st, a);
    else hipLaunchKernelGGL(k_seq_attention<64>, dim3((unsigned)blocks), dim3(64 * wpb), wpb * per_wave, st, a);
    return check_launch("k_seq_attention");
}

extern "C" int sss_add_layernorm(const float* x, int64_t ld_x, const float* res, int64_t ld_res, const float* gamma, const float* beta,
                                 float eps, int64_t n, int e, float* y, int64_t ld_y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (e < 4 || e % 4 || e > 1024 || !ok_ld(ld_x, e) || !ok_ld(ld_res, e) || !ok_ld(ld_y, e)) {
        set_error("add_layernorm: need e %% 4 == 0, 4 <= e <= 1024, leading dimensions %% 4 == 0 and >= e");
        return SSS_EINVAL;
    }
    if (!(eps > 0.f) || !ok_count(n)) { set_error("add_layernorm: need eps > 0 and 0 <= n < 2^31"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    if (!aligned16(x) || !aligned16(res) || !aligned16(gamma) || !aligned16(beta) || !aligned16(y)) {
        set_error("add_layernorm: need non-null 16-byte aligned x / res / gamma / beta / y");
        return SSS_EINVAL;
    }
    if (y == x && ld_y != ld_x) { set_error("add_layernorm: in place (y == x) needs ld_y == ld_x"); return SSS_EINVAL; }
    hipLaunchKernelGGL(k_add_layernorm, dim3(grid_blocks(n, 4, GRID_ALL)), dim3(256), 0, st, x, (long)ld_x, res, (long)ld_res, gamma, beta, eps,
                       (long)n, e, y, (long)ld_y);
    return check_launch("k_add_layernorm");
}

}  // namespace sss
