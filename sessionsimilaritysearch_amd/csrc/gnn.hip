// Session-encoder kernels, one per reference op (gfx950): HeteroGGNN message passing + positional-attention pooling at any
// width h % 4 == 0 -- the product path at the reference's h = 800; gnn_fused.hip holds the fused path of rows up to 256
// floats, linear.hip the GEMM (k_linear_grouped) of both.
//
// Reference ops replaced (op semantics Appendix A):
//   k_gat_aggregate     <- GATConv.propagate: leaky_relu(0.2) + per-target softmax + weighted sum
//                          + bias, over a CSR-by-target adjacency (model/gnn.py:54 via HeteroConv)
//   k_csr_weighted_sum  <- GatedGraphConv.propagate (aggr='add') (model/gnn.py:58)
//   k_gru_combine       <- torch.nn.GRUCell gate math + HeteroConv 'sum' + relu (model/gnn.py:59,72)
//   k_pool_expand / k_segment_pool <- PositionalAttentionPooling.forward (model/gnn.py:193-217)
//   k_segment_ptr       <- the per-graph row ranges of a sorted PyG `batch` vector
// Everything per-edge / per-node is HBM-bound and moves 16 B per lane.
#include "gnn_dev.h"

namespace sss {

// ------------------------------------------------------------------------------------------
// Per target node i (CSR by target): e_ij = leaky_relu(as[j] + ad[i], 0.2);
// w_ij = exp(e_ij - max_j e) / (sum_j exp(e_ij - max) + 1e-16); out[i] = sum_j w_ij xs[j] + bias
// (+ relu).  Targets without incoming edges get bias.  One group of LPR lanes per target, each
// lane owns float4 columns lane, lane+LPR, ... of the h-wide row.
template <int LPR>
__global__ __launch_bounds__(256) void k_gat_aggregate(
    const float* __restrict__ xs, long ld_xs, const float* __restrict__ a_src, long ld_as,
    const float* __restrict__ a_dst, long ld_ad, const int* __restrict__ rowptr,
    const int* __restrict__ col, long n_dst, int h, const float* __restrict__ bias, int relu,
    long n_self_loop, float* __restrict__ out, long ld_out) {
    const int sub = threadIdx.x % LPR;
    const long per_block = 256 / LPR;
    const int nv = h / 4;
    auto score = [&](long j, float ad) {
        const float v = a_src[j * ld_as] + ad;
        return v > 0.f ? v : 0.2f * v;
    };
    for (long i = (long)blockIdx.x * per_block + threadIdx.x / LPR; i < n_dst; i += (long)gridDim.x * per_block) {
        const int e0 = rowptr[i], e1 = rowptr[i + 1];
        const float ad = a_dst[i * ld_ad];
        // n_self_loop > 0: PyG's self-loop rewrite on the fly (drop source == target, append one i -> i)
        const long skip = n_self_loop > 0 ? i : -1, self = i < n_self_loop ? i : -1;
        float mx = -INFINITY;
        for (int e = e0; e < e1; ++e)
            if (col[e] != skip) mx = fmaxf(mx, score(col[e], ad));
        if (self >= 0) mx = fmaxf(mx, score(self, ad));
        float den = 0.f;
        for (int e = e0; e < e1; ++e)
            if (col[e] != skip) den += expf(score(col[e], ad) - mx);
        if (self >= 0) den += expf(score(self, ad) - mx);
        const float inv = 1.f / (den + 1e-16f);
        for (int c = sub; c < nv; c += LPR) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            auto add = [&](long j) {
                const float w = expf(score(j, ad) - mx) * inv;
                const float4 x = *reinterpret_cast<const float4*>(xs + j * ld_xs + c * 4);
                acc.x += w * x.x; acc.y += w * x.y; acc.z += w * x.z; acc.w += w * x.w;
            };
            for (int e = e0; e < e1; ++e)
                if (col[e] != skip) add(col[e]);
            if (self >= 0) add(self);
            if (bias) {
                const float4 b = *reinterpret_cast<const float4*>(bias + c * 4);
                acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
            }
            if (relu) {
                acc.x = fmaxf(acc.x, 0.f); acc.y = fmaxf(acc.y, 0.f);
                acc.z = fmaxf(acc.z, 0.f); acc.w = fmaxf(acc.w, 0.f);
            }
            *reinterpret_cast<float4*>(out + i * ld_out + c * 4) = acc;
        }
    }
}

// out[i] = sum_{e in row i} (w[e] *) m[col[e]]   (GatedGraphConv aggregate, aggr='add')
template <int LPR>
__global__ __launch_bounds__(256) void k_csr_weighted_sum(const float* __restrict__ m, long ld_m,
                                                          const int* __restrict__ rowptr,
                                                          const int* __restrict__ col,
                                                          const float* __restrict__ w, long n_dst, int h,
                                                          float* __restrict__ out, long ld_out) {
    const int sub = threadIdx.x % LPR;
    const long per_block = 256 / LPR;
    const int nv = h / 4;
    for (long i = (long)blockIdx.x * per_block + threadIdx.x / LPR; i < n_dst; i += (long)gridDim.x * per_block) {
        const int e0 = rowptr[i], e1 = rowptr[i + 1];
        for (int c = sub; c < nv; c += LPR) {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int e = e0; e < e1; ++e) {
                const float4 x = *reinterpret_cast<const float4*>(m + (long)col[e] * ld_m + c * 4);
                const float ww = w ? w[e] : 1.f;
                acc.x += ww * x.x; acc.y += ww * x.y; acc.z += ww * x.z; acc.w += ww * x.w;
            }
            *reinterpret_cast<float4*>(out + i * ld_out + c * 4) = acc;
        }
    }
}

// GRUCell(input = aggregated message, hidden = x) + the GAT term + relu:
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r * gh_n), h' = (1 - z) n + z x
//   out = relu(add + h')        gi / gh already contain b_ih / b_hh.  x is zero-padded to h.
// (SSS_GRU1 here and in k_layer_update, gnn_fused.hip, are two macros on purpose: this one adds add + ((1 - z) n + z x),
// that one (t1 + (1 - z) n) + z x -- one macro for both would move the last bit of one of them.)
__global__ __launch_bounds__(256) void k_gru_combine(const float* __restrict__ gi, long ld_gi,
                                                     const float* __restrict__ gh, long ld_gh,
                                                     const float* __restrict__ x, long ld_x, int d_x,
                                                     const float* __restrict__ add, long ld_add, long n,
                                                     int h, float* __restrict__ out, long ld_out) {
    const int nv = h / 4;
    const long total = n * nv;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long i = idx / nv;
        const int c = (int)(idx % nv) * 4;
        const float4 ir = *reinterpret_cast<const float4*>(gi + i * ld_gi + c);
        const float4 iz = *reinterpret_cast<const float4*>(gi + i * ld_gi + h + c);
        const float4 in = *reinterpret_cast<const float4*>(gi + i * ld_gi + 2 * h + c);
        const float4 hr = *reinterpret_cast<const float4*>(gh + i * ld_gh + c);
        const float4 hz = *reinterpret_cast<const float4*>(gh + i * ld_gh + h + c);
        const float4 hn = *reinterpret_cast<const float4*>(gh + i * ld_gh + 2 * h + c);
        float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c + 3 < d_x) xv = *reinterpret_cast<const float4*>(x + i * ld_x + c);
        else {
            if (c + 0 < d_x) xv.x = x[i * ld_x + c + 0];
            if (c + 1 < d_x) xv.y = x[i * ld_x + c + 1];
            if (c + 2 < d_x) xv.z = x[i * ld_x + c + 2];
        }
        const float4 av = add ? *reinterpret_cast<const float4*>(add + i * ld_add + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 o;
#define SSS_GRU1(f)                                                        \
    {                                                                      \
        const float rr = sigmoidf_(ir.f + hr.f);                           \
        const float zz = sigmoidf_(iz.f + hz.f);                           \
        const float nn = tanhf(in.f + rr * hn.f);                          \
        const float hp = (1.f - zz) * nn + zz * xv.f;                      \
        o.f = fmaxf(av.f + hp, 0.f);                                       \
    }
        SSS_GRU1(x) SSS_GRU1(y) SSS_GRU1(z) SSS_GRU1(w)
#undef SSS_GRU1
        *reinterpret_cast<float4*>(out + i * ld_out + c) = o;
    }
}

// ---------------------------------------------------------------------------- pooling pieces
// Expanded pooling nodes (product clicks first, then queries), model/gnn.py:199-208:
//   node[e, 0:Dl] = tanh(lin[src_row[e], 0:Dl]),  node[e, Dl:Dl+P] = tanh(pos_emb[pos_id[e], :])
__global__ __launch_bounds__(256) void k_pool_expand(const float* __restrict__ lin_p, const float* __restrict__ lin_q,
                                                     long ld_lin, const int* __restrict__ src_row,
                                                     const int* __restrict__ pos_id, long n_clicks, long n_exp,
                                                     int Dl, int P, const float* __restrict__ pos_emb,
                                                     float* __restrict__ node, long ld_node) {
    const int D = Dl + P;
    const long total = n_exp * D;
    for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
        const long e = idx / D;
        const int c = (int)(idx % D);
        float v;
        if (c < Dl) {
            const float* lin = e < n_clicks ? lin_p : lin_q;
            v = lin[(long)src_row[e] * ld_lin + c];
        } else {
            v = pos_emb[(long)pos_id[e] * P + (c - Dl)];
        }
        node[e * ld_node + c] = tanhf(v);
    }
}

// mean over the expanded nodes of graph g: product-click rows [pptr[g], pptr[g+1]) and query rows
// n_clicks + [qptr[g], qptr[g+1]) (global_mean_pool, Appendix A.4).  One LPR-lane group per graph.
// weight == nullptr: plain mean.  Otherwise the attention-weighted mean of model/gnn.py:214-217:
//   att_n = sum_c watt[c] * sigmoid(A[n, c] + bcoarse[g, c]);  out[g] = mean_n(node[n] * att_n)
template <int LPR>
__global__ __launch_bounds__(256) void k_segment_pool(const float* __restrict__ node, long ld_node,
                                                      const int* __restrict__ pptr, const int* __restrict__ qptr,
                                                      long n_clicks, long n_graphs, int D,
                                                      const float* __restrict__ A, long ld_a,
                                                      const float* __restrict__ bcoarse, long ld_b,
                                                      const float* __restrict__ watt,
                                                      float* __restrict__ out, long ld_out, int reduce_sum = 0) {
    const int sub = threadIdx.x % LPR;
    const long per_block = 256 / LPR;
    const int nv = D / 4;
    for (long g = (long)blockIdx.x * per_block + threadIdx.x / LPR; g < n_graphs; g += (long)gridDim.x * per_block) {
        const int p0 = pptr[g], p1 = pptr[g + 1], q0 = qptr[g], q1 = qptr[g + 1];
        const int cnt = (p1 - p0) + (q1 - q0);
        const float invc = reduce_sum ? 1.f : 1.f / (float)(cnt > 0 ? cnt : 1);     // sum: SRGNN_Pooling's global_add_pool
        // Wide rows with attention (the reference's D = 1600: 400 float4 columns over 64 lanes): ONE sweep over the
        // graph's nodes -- a node's attention weight is computed once and applied to all of the lane's (up to eight)
        // columns; the column-chunked sweeps below would recompute it, and re-read the node's A row, per chunk.
        // Same additions in the same order per output element.
        if (watt && nv > 2 * LPR && nv <= 8 * LPR) {
            float4 acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < cnt; ++t) {
                const long nrow = t < (p1 - p0) ? (long)(p0 + t) : n_clicks + (long)(q0 + t - (p1 - p0));
                float part = 0.f;
                for (int c = sub; c < nv; c += LPR) {
                    const float4 a = *reinterpret_cast<const float4*>(A + nrow * ld_a + c * 4);
                    const float4 b = *reinterpret_cast<const float4*>(bcoarse + g * ld_b + c * 4);
                    const float4 w = *reinterpret_cast<const float4*>(watt + c * 4);
                    part += w.x * sigmoidf_(a.x + b.x) + w.y * sigmoidf_(a.y + b.y) +
                            w.z * sigmoidf_(a.z + b.z) + w.w * sigmoidf_(a.w + b.w);
                }
                part = group_sum<LPR>(part);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int c = sub + j * LPR;
                    if (c < nv) {
                        const float4 v = *reinterpret_cast<const float4*>(node + nrow * ld_node + c * 4);
                        acc[j].x += part * v.x; acc[j].y += part * v.y; acc[j].z += part * v.z; acc[j].w += part * v.w;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = sub + j * LPR;
                if (c < nv)
                    *reinterpret_cast<float4*>(out + g * ld_out + c * 4) =
                        make_float4(acc[j].x * invc, acc[j].y * invc, acc[j].z * invc, acc[j].w * invc);
            }
            continue;
        }
        // two float4 columns per lane per sweep (named accumulators, never runtime-indexed);
        // rows wider than 8 * LPR floats take several sweeps over the graph's nodes
        for (int cb = 0; cb < nv; cb += 2 * LPR) {
            const int c0 = cb + sub, c1 = cb + sub + LPR;
            float4 acc0 = make_float4(0.f, 0.f, 0.f, 0.f), acc1 = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int t = 0; t < cnt; ++t) {
                const long nrow = t < (p1 - p0) ? (long)(p0 + t) : n_clicks + (long)(q0 + t - (p1 - p0));
                float att = 1.f;
                if (watt) {
                    float part = 0.f;
                    for (int c = sub; c < nv; c += LPR) {
                        const float4 a = *reinterpret_cast<const float4*>(A + nrow * ld_a + c * 4);
                        const float4 b = *reinterpret_cast<const float4*>(bcoarse + g * ld_b + c * 4);
                        const float4 w = *reinterpret_cast<const float4*>(watt + c * 4);
                        part += w.x * sigmoidf_(a.x + b.x) + w.y * sigmoidf_(a.y + b.y) +
                                w.z * sigmoidf_(a.z + b.z) + w.w * sigmoidf_(a.w + b.w);
                    }
                    att = group_sum<LPR>(part);
                }
                if (c0 < nv) {
                    const float4 v = *reinterpret_cast<const float4*>(node + nrow * ld_node + c0 * 4);
                    acc0.x += att * v.x; acc0.y += att * v.y; acc0.z += att * v.z; acc0.w += att * v.w;
                }
                if (c1 < nv) {
                    const float4 v = *reinterpret_cast<const float4*>(node + nrow * ld_node + c1 * 4);
                    acc1.x += att * v.x; acc1.y += att * v.y; acc1.z += att * v.z; acc1.w += att * v.w;
                }
            }
            if (c0 < nv)
                *reinterpret_cast<float4*>(out + g * ld_out + c0 * 4) =
                    make_float4(acc0.x * invc, acc0.y * invc, acc0.z * invc, acc0.w * invc);
            if (c1 < nv)
                *reinterpret_cast<float4*>(out + g * ld_out + c1 * 4) =
                    make_float4(acc1.x * invc, acc1.y * invc, acc1.z * invc, acc1.w * invc);
        }
    }
}

// ptr[g] = first index i with batch[i] >= g (batch sorted ascending), g in [0, n_graphs]
__global__ void k_segment_ptr(const long* __restrict__ batch, long n, long n_graphs, int* __restrict__ ptr) {
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > n_graphs) return;
    long lo = 0, hi = n;
    while (lo < hi) {
        const long mid = (lo + hi) >> 1;
        if (batch[mid] < g) lo = mid + 1; else hi = mid;
    }
    ptr[g] = (int)lo;
}

// ------------------------------------------------------------------------------ host launchers
// the lane-group kernels here grid-stride over their rows: at most 4096 workgroups
constexpr long GRID_CAP = 4096;

extern "C" int sss_gat_aggregate(const float* xs, int64_t ld_xs, const float* a_src, int64_t ld_as, const float* a_dst, int64_t ld_ad,
                                 const int32_t* rowptr, const int32_t* col, int64_t n_dst, int h, const float* bias, int relu,
                                 int64_t n_self_loop, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_dst < 0 || h <= 0 || h % 4 || ld_xs % 4 || ld_out % 4 || ld_out < h) {
        set_error("gat_aggregate: need h %% 4 == 0 and 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_dst == 0) return SSS_OK;
    SSS_LPR_SWITCH(lanes_for(h), hipLaunchKernelGGL(k_gat_aggregate<L>, dim3(grid_blocks(n_dst, 256 / L, GRID_CAP)), dim3(256), 0, st,
                                                    xs, ld_xs, a_src, ld_as, a_dst, ld_ad, rowptr, col, n_dst, h, bias, relu,
                                                    n_self_loop, out, ld_out));
    return check_launch("k_gat_aggregate");
}

extern "C" int sss_csr_weighted_sum(const float* m, int64_t ld_m, const int32_t* rowptr, const int32_t* col, const float* w,
                                    int64_t n_dst, int h, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_dst < 0 || h <= 0 || h % 4 || ld_m % 4 || ld_out % 4 || ld_out < h) {
        set_error("csr_weighted_sum: need h %% 4 == 0 and 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_dst == 0) return SSS_OK;
    SSS_LPR_SWITCH(lanes_for(h), hipLaunchKernelGGL(k_csr_weighted_sum<L>, dim3(grid_blocks(n_dst, 256 / L, GRID_CAP)), dim3(256), 0,
                                                    st, m, ld_m, rowptr, col, w, n_dst, h, out, ld_out));
    return check_launch("k_csr_weighted_sum");
}

extern "C" int sss_gru_combine(const float* gi, int64_t ld_gi, const float* gh, int64_t ld_gh, const float* x, int64_t ld_x, int d_x,
                               const float* add, int64_t ld_add, int64_t n, int h, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || h <= 0 || h % 4 || d_x > h || ld_gi % 4 || ld_gh % 4 || ld_out % 4 || (add && ld_add % 4) ||
        (d_x >= 4 && ld_x % 4)) {
        set_error("gru_combine: need h %% 4 == 0, d_x <= h and 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_gru_combine, dim3(grid_blocks(n * (h / 4), 256, GRID_CAP)), dim3(256), 0, st, gi, ld_gi, gh, ld_gh, x, ld_x,
                       d_x, add, ld_add, n, h, out, ld_out);
    return check_launch("k_gru_combine");
}

extern "C" int sss_pool_expand(const float* lin_p, const float* lin_q, int64_t ld_lin, const int32_t* src_row, const int32_t* pos_id,
                               int64_t n_clicks, int64_t n_exp, int d_lin, int p, const float* pos_emb, float* node, int64_t ld_node,
                               void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_exp < 0 || n_clicks < 0 || n_clicks > n_exp || d_lin <= 0 || p < 0 || ld_node < d_lin + p) {
        set_error("pool_expand: bad arguments");
        return SSS_EINVAL;
    }
    if (n_exp == 0) return SSS_OK;
    hipLaunchKernelGGL(k_pool_expand, dim3(grid_blocks(n_exp * (d_lin + p), 256, GRID_CAP)), dim3(256), 0, st, lin_p, lin_q, ld_lin,
                       src_row, pos_id, n_clicks, n_exp, d_lin, p, pos_emb, node, ld_node);
    return check_launch("k_pool_expand");
}

int launch_segment_pool(const float* node, long ld_node, const int* pptr, const int* qptr, long n_clicks, long n_graphs, int d,
                        const float* a, long ld_a, const float* bcoarse, long ld_b, const float* watt, float* out, long ld_out,
                        int reduce_sum, hipStream_t st) {
    SSS_LPR_SWITCH(lanes_for(d), hipLaunchKernelGGL(k_segment_pool<L>, dim3(grid_blocks(n_graphs, 256 / L, GRID_CAP)), dim3(256), 0, st,
                                                    node, ld_node, pptr, qptr, n_clicks, n_graphs, d, a, ld_a, bcoarse, ld_b, watt,
                                                    out, ld_out, reduce_sum));
    return check_launch("k_segment_pool");
}

extern "C" int sss_segment_pool(const float* node, int64_t ld_node, const int32_t* pptr, const int32_t* qptr, int64_t n_clicks,
                                int64_t n_graphs, int d, const float* a, int64_t ld_a, const float* bcoarse, int64_t ld_b,
                                const float* watt, float* out, int64_t ld_out, void* stream) {
    if (n_graphs < 0 || d <= 0 || d % 4 || ld_node % 4 || ld_out % 4 ||
        (watt && (!a || !bcoarse || ld_a % 4 || ld_b % 4))) {
        set_error("segment_pool: need D %% 4 == 0 and 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_graphs == 0) return SSS_OK;
    return launch_segment_pool(node, ld_node, pptr, qptr, n_clicks, n_graphs, d, a, ld_a, bcoarse, ld_b, watt, out, ld_out, 0,
                               static_cast<hipStream_t>(stream));
}

extern "C" int sss_segment_ptr(const int64_t* batch, int64_t n, int64_t n_graphs, int32_t* ptr, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || n_graphs < 0) { set_error("segment_ptr: bad arguments"); return SSS_EINVAL; }
    hipLaunchKernelGGL(k_segment_ptr, dim3((unsigned)((n_graphs + 1 + 255) / 256)), dim3(256), 0, st, batch, n, n_graphs, ptr);
    return check_launch("k_segment_ptr");
}

}  // namespace sss
