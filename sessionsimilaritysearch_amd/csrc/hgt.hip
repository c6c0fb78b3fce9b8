// HGTConv's attention aggregation on CSR by target (gfx950; include/sss_hgt.h states the computation, DESIGN.md
// section 5.8 derives it from PyG's HGTConv -- the reference's HGT, model/gnn.py:9-41).  HBM / L2-bound row kernels in the
// shape of k_csr_mean and k_gat_aggregate: one LPR-lane group per TARGET node, 16 bytes per lane per access.
//   k_hgt_aggregate  multi-head dot-product attention over one or two edge-type slots, softmax per slot and head,
//                    slots summed, optional exact gelu on the way out
//   k_hgt_skip       y += beta * x, the (1 - sigmoid(skip)) x half of the layer's skip connection
// Lane map of k_hgt_aggregate: LPR = the power of two >= heads * D / 4, at most 64.  Head eta owns the LH = LPR / heads
// lanes [eta LH, (eta + 1) LH) of the group; lane s of a head walks the head's float4 columns s, s + LH, s + 2 LH, ...
// (NCH of them; columns past D are predicated off: D = 200 leaves the fourth step to 2 of 16 lanes).  Rows wider than 256
// floats take LPR = 64 -- one wave per target -- and NCH = 2, 4 or 8; 8 x float4 each of q, the accumulator, the slot sum
// and the k | v pair in flight is the register bound behind heads * D <= 2048.
#include <math.h>

#include "lane_group.h"
#include "../../include/sss_hgt.h"

namespace sss {

template <int LPR, int NCH>
__global__ __launch_bounds__(256) void k_hgt_aggregate(const sss_hgt_args A) {
    const int sub = threadIdx.x % LPR;
    const long i = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int LH = LPR / A.heads, D = A.head_dim;
    const int s = sub % LH, hoff = (sub / LH) * D;
    const bool in = i < A.n_dst;                             // no early return: the shuffles below stay convergent
    bool ok[NCH];
    float4 q[NCH], res[NCH];
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        const int c = (s + j * LH) * 4;
        ok[j] = in && c < D;
        q[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        res[j] = q[j];
        if (ok[j]) q[j] = *reinterpret_cast<const float4*>(A.q + i * A.ld_q + hoff + c);
    }
    for (int sl = 0; sl < A.n_slots; ++sl) {
        const sss_hgt_slot S = A.slot[sl];
        int e0 = 0, cnt = 0;
        if (in) { e0 = S.rowptr[i]; cnt = S.rowptr[i + 1] - e0; }
        int cmax = cnt;                                      // the groups of one wave may differ in degree
        if (LPR < 64) {
#pragma unroll
            for (int o = 32; o >= LPR; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o));
        }
        // one pass (online softmax, the idiom of gat_row in gnn_fused.hip): a new maximum rescales what has been summed so
        // far, so every edge's index and k | v row are loaded exactly once
        float mx = -INFINITY, den = 0.f;
        float4 acc[NCH];
#pragma unroll
        for (int j = 0; j < NCH; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        long src = cnt > 0 ? S.col[e0] : 0;
        for (int t = 0; t < cmax; ++t) {
            const bool live = t < cnt;
            const long cur = src;
            if (t + 1 < cnt) src = S.col[e0 + t + 1];        // the next edge's index flies under this edge's rows
            float4 kk[NCH], vv[NCH];
            float part = 0.f;
#pragma unroll
            for (int j = 0; j < NCH; ++j) {
                const int c = hoff + (s + j * LH) * 4;
                kk[j] = make_float4(0.f, 0.f, 0.f, 0.f);
                vv[j] = kk[j];
                if (live && ok[j]) {
                    kk[j] = *reinterpret_cast<const float4*>(S.k + cur * S.ld_k + c);
                    vv[j] = *reinterpret_cast<const float4*>(S.v + cur * S.ld_v + c);
                }
            }
#pragma unroll
            for (int j = 0; j < NCH; ++j) part += q[j].x * kk[j].x + q[j].y * kk[j].y + q[j].z * kk[j].z + q[j].w * kk[j].w;
            for (int o = LH >> 1; o > 0; o >>= 1) part += __shfl_xor(part, o);       // the head's dot, in all its lanes
            if (live) {
                if (part > mx) {
                    const float sc = expf(mx - part);        // exp(-inf) = 0 on the first edge
                    den *= sc;
#pragma unroll
                    for (int j = 0; j < NCH; ++j) { acc[j].x *= sc; acc[j].y *= sc; acc[j].z *= sc; acc[j].w *= sc; }
                    mx = part;
                }
                const float ex = expf(part - mx);
                den += ex;
#pragma unroll
                for (int j = 0; j < NCH; ++j) {
                    acc[j].x += ex * vv[j].x; acc[j].y += ex * vv[j].y; acc[j].z += ex * vv[j].z; acc[j].w += ex * vv[j].w;
                }
            }
        }
        const float inv = 1.f / (den + 1e-16f);              // no edge: acc = 0, so zeros
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            res[j].x += acc[j].x * inv; res[j].y += acc[j].y * inv; res[j].z += acc[j].z * inv; res[j].w += acc[j].w * inv;
        }
    }
#pragma unroll
    for (int j = 0; j < NCH; ++j) {
        if (!ok[j]) continue;
        float4 o = res[j];
        if (A.gelu) o = make_float4(gelu_erf(o.x), gelu_erf(o.y), gelu_erf(o.z), gelu_erf(o.w));
        *reinterpret_cast<float4*>(A.out + i * A.ld_out + hoff + (s + j * LH) * 4) = o;
    }
}

__global__ __launch_bounds__(256) void k_hgt_skip(float* __restrict__ y, long ld_y, const float* __restrict__ x, long ld_x,
                                                  float beta, long n, int h4) {
    const long total = n * h4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / h4;
        const int c = (int)(idx % h4) * 4;
        float4 a = *reinterpret_cast<const float4*>(y + r * ld_y + c);
        const float4 b = *reinterpret_cast<const float4*>(x + r * ld_x + c);
        a.x += beta * b.x; a.y += beta * b.y; a.z += beta * b.z; a.w += beta * b.w;
        *reinterpret_cast<float4*>(y + r * ld_y + c) = a;
    }
}

// one lane group per target, no grid-stride: every target gets its group
#define SSS_HGT_LAUNCH(L, N) \
    hipLaunchKernelGGL((k_hgt_aggregate<L, N>), dim3(grid_blocks(a.n_dst, 256 / L, GRID_ALL)), dim3(256), 0, st, a)

extern "C" int sss_hgt_aggregate(const sss_hgt_args* args, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!args) { set_error("hgt_aggregate: null args"); return SSS_EINVAL; }
    const sss_hgt_args a = *args;
    if (a.n_slots < 1 || a.n_slots > 2) { set_error("hgt_aggregate: one or two edge-type slots, got %d", a.n_slots); return SSS_EINVAL; }
    if (a.heads != 1 && a.heads != 2 && a.heads != 4 && a.heads != 8) { set_error("hgt_aggregate: heads must be 1, 2, 4 or 8, got %d", a.heads); return SSS_EINVAL; }
    if (a.head_dim <= 0 || a.head_dim % 4 || (long)a.heads * a.head_dim > 2048) {
        set_error("hgt_aggregate: need head_dim %% 4 == 0 and heads * head_dim <= 2048, got %d x %d", a.heads, a.head_dim);
        return SSS_EINVAL;
    }
    if (!ok_count(a.n_dst)) { set_error("hgt_aggregate: need 0 <= n_dst < 2^31"); return SSS_EINVAL; }
    if (a.n_dst == 0) return SSS_OK;
    const int width = a.heads * a.head_dim;
    bool ok = aligned16(a.q) && aligned16(a.out) && ok_ld(a.ld_q, width) && ok_ld(a.ld_out, width);
    for (int i = 0; i < a.n_slots; ++i) {
        const sss_hgt_slot& s = a.slot[i];
        ok = ok && aligned16(s.k) && aligned16(s.v) && s.rowptr && s.col && ok_ld(s.ld_k, width) && ok_ld(s.ld_v, width);
    }
    if (!ok) { set_error("hgt_aggregate: need non-null 16-byte aligned q / k / v / out, non-null rowptr / col, leading dimensions %% 4 == 0 and >= heads * head_dim"); return SSS_EINVAL; }
    const int lpr = lanes_for(width);
    const int lh = lpr / a.heads;                            // >= 1: width / 4 >= heads
    const int steps = (a.head_dim / 4 + lh - 1) / lh;        // float4 columns per lane: 1 below 64 lanes, <= 8 at 64
    if (lpr < 64 || steps <= 1) { SSS_LPR_SWITCH(lpr, SSS_HGT_LAUNCH(L, 1)); }
    else if (steps <= 2) SSS_HGT_LAUNCH(64, 2);
    else if (steps <= 4) SSS_HGT_LAUNCH(64, 4);
    else SSS_HGT_LAUNCH(64, 8);
    return check_launch("k_hgt_aggregate");
}
#undef SSS_HGT_LAUNCH

extern "C" int sss_hgt_skip(float* y, int64_t ld_y, const float* x, int64_t ld_x, float beta, int64_t n, int h, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (h <= 0 || h % 4 || !ok_count(n)) { set_error("hgt_skip: need h %% 4 == 0 and 0 <= n < 2^31"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    if (!aligned16(y) || !aligned16(x) || !ok_ld(ld_y, h) || !ok_ld(ld_x, h)) {
        set_error("hgt_skip: need non-null 16-byte aligned y / x, leading dimensions %% 4 == 0 and >= h");
        return SSS_EINVAL;
    }
    hipLaunchKernelGGL(k_hgt_skip, dim3(grid_blocks(n * (h / 4), 256, 1 << 20)), dim3(256), 0, st, y, ld_y, x, ld_x, beta, (long)n, h / 4);
    return check_launch("k_hgt_skip");
}

}  // namespace sss
