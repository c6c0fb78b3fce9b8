// Fused session-encoder path for rows of at most 256 floats (gfx950; 8 launches per forward with the GEMMs of linear.hip;
// DESIGN.md "encoder").  gnn.hip holds the per-op kernels of any width.
//   gat_row             the GAT segment softmax of one target, single pass (device function)
//   k_layer_update      per target node: GAT segment-softmax aggregate + GatedGraphConv aggregate +
//                       GRU gates + HeteroConv sum + relu, everything in registers
//   k_pool_expand_mean  tanh([lin ; pos]) rows + per-graph mean
//   k_pool_attention    attention-weighted per-graph mean (+ optional L2 normalise)
//   k_pool_attention_tab  the same pooling without materialising the expanded rows
// The node-linear inputs come from k_linear_grouped (linear.hip): one launch for up to 4 problems (products + queries of a
// layer, or the pooling's lin_p + lin_q, or node_lin + coarse_lin); layer 0 reads its X rows straight from the feature
// tables (NodeAsinEmbedding gather fused in).
#include "gnn_dev.h"

namespace sss {

// ------------------------------------------------------------------------------------------
// One LPR-lane group per TARGET node (LPR = h / 4: a lane owns one float4 column of the h-wide
// row).  Targets [0, Np) are products, [Np, Np + Nq) queries.
//   product i:  t1 = GAT(query -> product)  (Appendix A.2: leaky_relu(0.2), per-target softmax,
//                    + 1e-16 in the denominator, + bias)
//               gi = sum_{j -> i} w_ij u[j] + b_ih   with u = x (W_g W_ih^T): the GatedGraphConv
//                    message transform and the GRU input transform applied BEFORE the (linear)
//                    aggregation, so no second GEMM is needed (Appendix A.3)
//               out = relu(t1 + (1 - z) n + z x),  r, z, n = GRU gates of (gi, gh = W_hh x + b_hh)
//   query i:    out = relu(GAT(product -> query))
// Column layout of the node-linear outputs (written by k_linear_grouped, see encoder.py):
//   Yp [Np, 7h+32]: xs_p | u_r u_z u_n | gh_r gh_z gh_n | a_src(pq) a_dst(qp)
//   Yq [Nq,  h+32]: xs_q | a_src(qp) a_dst(pq)

__device__ __forceinline__ float4 f4_fma(float w, float4 x, float4 a) {
    a.x += w * x.x; a.y += w * x.y; a.z += w * x.z; a.w += w * x.w;
    return a;
}
__device__ __forceinline__ float leaky02(float v) { return v > 0.f ? v : 0.2f * v; }

// softmax-weighted sum over the incoming edges of one target: returns sum_e softmax_e * xs[col[e]][c4] + bias.
// self_i >= 0 applies PyG's GATConv(add_self_loops=True) edge rewrite on the fly (Appendix A.2):
// edges whose source index equals the target index are dropped and ONE edge self_i -> target is
// appended after the target's other edges (what remove_self_loops + add_self_loops + a stable
// sort by target produce).
__device__ __forceinline__ float4 gat_row(const float* xs, long ld, const float* a_src_col, float ad, const int* col,
                                          int e0, int e1, int c4, const float* bias, long skip_i, long self_i,
                                          const long* row_of = nullptr) {
    // one pass (online softmax): a new maximum rescales what has been summed so far, so every
    // edge's index / score / row is loaded exactly once
    float mx = -INFINITY, den = 0.f;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    auto edge = [&](long jn) {
        const long j = row_of ? row_of[jn] : jn;           // table mode: the source node's table row
        const float v = leaky02(a_src_col[j * ld] + ad);
        const float4 x = *reinterpret_cast<const float4*>(xs + j * ld + c4);
        if (v > mx) {
            const float sc = expf(mx - v);                 // exp(-inf) = 0 on the first edge
            den *= sc; acc.x *= sc; acc.y *= sc; acc.z *= sc; acc.w *= sc;
            mx = v;
        }
        const float ex = expf(v - mx);
        den += ex;
        acc = f4_fma(ex, x, acc);
    };
    for (int e = e0; e < e1; ++e) {
        const long j = col[e];
        if (j != skip_i) edge(j);
    }
    if (self_i >= 0) edge(self_i);
    const float inv = 1.f / (den + 1e-16f);
    const float4 b = *reinterpret_cast<const float4*>(bias + c4);
    return make_float4(acc.x * inv + b.x, acc.y * inv + b.y, acc.z * inv + b.z, acc.w * inv + b.w);
}

// The argument is the C ABI's own struct (sss_layer_args, include/sss.h, where table mode -- row_p / row_q, x0_p / x0_q --
// is described).
template <int LPR>
__global__ __launch_bounds__(256) void k_layer_update(const sss_layer_args A) {
    const int sub = threadIdx.x % LPR;
    const long per_block = 256 / LPR;
    const long t = (long)blockIdx.x * per_block + threadIdx.x / LPR;
    const int h = A.h, c4 = sub * 4;
    if (c4 >= h || t >= A.np + A.nq) return;
    if (t >= A.np) {                                            // ---- query target
        const long i = t - A.np;
        const long ri = A.row_q ? A.row_q[i] : i;
        const float ad = A.yq[ri * A.ld_yq + h + 1];
        const bool lp = i < A.n_self_loop;
        float4 o = gat_row(A.yp, A.ld_yp, A.yp + 7 * h, ad, A.col_pq, A.rowptr_pq[i], A.rowptr_pq[i + 1], c4, A.bias_pq,
                           A.n_self_loop > 0 ? i : -1, lp ? i : -1, A.row_p);
        if (A.x0_q) {                                           // raw query features -> slice 0 of the node buffer
            const float* xq = A.xq_table + ri * A.ld_xq;
            float* dq = A.x0_q + i * A.ld_x0_q;
            if (c4 + 3 < A.d_x) *reinterpret_cast<float4*>(dq + c4) = *reinterpret_cast<const float4*>(xq + c4);
            else for (int u = 0; u < 4; ++u) if (c4 + u < A.d_x) dq[c4 + u] = xq[c4 + u];
        }
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
        *reinterpret_cast<float4*>(A.out_q + i * A.ld_out_q + c4) = o;
        return;
    }
    const long i = t;                                           // ---- product target
    const long ri = A.row_p ? A.row_p[i] : i;
    const float* yi = A.yp + ri * A.ld_yp;
    const float4 t1 = gat_row(A.yq, A.ld_yq, A.yq + h, yi[7 * h + 1], A.col_qp, A.rowptr_qp[i], A.rowptr_qp[i + 1], c4, A.bias_qp,
                              A.n_self_loop > 0 ? i : -1, i < A.n_self_loop ? i : -1, A.row_q);
    float4 gr = *reinterpret_cast<const float4*>(A.b_ih + c4);
    float4 gz = *reinterpret_cast<const float4*>(A.b_ih + h + c4);
    float4 gn = *reinterpret_cast<const float4*>(A.b_ih + 2 * h + c4);
    for (int e = A.rowptr_pp[i]; e < A.rowptr_pp[i + 1]; ++e) {
        const long jn = A.col_pp[e];
        const float* uj = A.yp + (A.row_p ? A.row_p[jn] : jn) * A.ld_yp + h + c4;
        const float w = A.w_pp ? A.w_pp[e] : 1.f;
        gr = f4_fma(w, *reinterpret_cast<const float4*>(uj), gr);
        gz = f4_fma(w, *reinterpret_cast<const float4*>(uj + h), gz);
        gn = f4_fma(w, *reinterpret_cast<const float4*>(uj + 2 * h), gn);
    }
    const float4 hr = *reinterpret_cast<const float4*>(yi + 4 * h + c4);
    const float4 hz = *reinterpret_cast<const float4*>(yi + 5 * h + c4);
    const float4 hn = *reinterpret_cast<const float4*>(yi + 6 * h + c4);
    float4 xv = make_float4(0.f, 0.f, 0.f, 0.f);
    const float* xi = A.xin_p + ri * A.ld_xin;
    if (c4 + 3 < A.d_x) xv = *reinterpret_cast<const float4*>(xi + c4);
    else {
        if (c4 + 0 < A.d_x) xv.x = xi[c4 + 0];
        if (c4 + 1 < A.d_x) xv.y = xi[c4 + 1];
        if (c4 + 2 < A.d_x) xv.z = xi[c4 + 2];
    }
    if (A.x0_p) {                                               // raw product features -> slice 0 of the node buffer
        float* dp = A.x0_p + i * A.ld_x0_p;
        if (c4 + 3 < A.d_x) *reinterpret_cast<float4*>(dp + c4) = xv;
        else {
            if (c4 + 0 < A.d_x) dp[c4 + 0] = xv.x;
            if (c4 + 1 < A.d_x) dp[c4 + 1] = xv.y;
            if (c4 + 2 < A.d_x) dp[c4 + 2] = xv.z;
        }
    }
    float4 o;
    // (not the SSS_GRU1 of k_gru_combine, gnn.hip: this one adds (t1 + (1 - z) n) + z x, that one add + ((1 - z) n + z x))
#define SSS_GRU1(f)                                                        \
    {                                                                      \
        const float rr = sigmoidf_(gr.f + hr.f);                           \
        const float zz = sigmoidf_(gz.f + hz.f);                           \
        const float nn = tanhf(gn.f + rr * hn.f);                          \
        o.f = fmaxf(t1.f + (1.f - zz) * nn + zz * xv.f, 0.f);              \
    }
    SSS_GRU1(x) SSS_GRU1(y) SSS_GRU1(z) SSS_GRU1(w)
#undef SSS_GRU1
    *reinterpret_cast<float4*>(A.out_p + i * A.ld_out_p + c4) = o;
}

// ------------------------------------------------------------------------------------------
// PositionalAttentionPooling, first half (model/gnn.py:195-211): one LPR-lane group per graph g
// walks its expanded rows (product clicks [pptr[g], pptr[g+1]), then query rows
// n_clicks + [qptr[g], qptr[g+1])), writes node[e] = tanh([lin[src_row[e]] ; pos_emb[pos_id[e]]])
// and the graph mean coarse[g] (global_mean_pool).
template <int LPR>
__global__ __launch_bounds__(256) void k_pool_expand_mean(const float* __restrict__ lin_p, const float* __restrict__ lin_q,
                                                          long ld_lin, const int* __restrict__ src_row,
                                                          const int* __restrict__ pos_id, const int* __restrict__ pptr,
                                                          const int* __restrict__ qptr, long n_clicks, long n_graphs,
                                                          int Dl, int P, const float* __restrict__ pos_emb,
                                                          float* __restrict__ node, long ld_node,
                                                          float* __restrict__ coarse, long ld_coarse) {
    const int sub = threadIdx.x % LPR;
    const long g = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int D = Dl + P, c4 = sub * 4;
    if (g >= n_graphs || c4 >= D) return;
    const int p0 = pptr[g], p1 = pptr[g + 1], q0 = qptr[g], q1 = qptr[g + 1];
    const int np_ = p1 - p0, cnt = np_ + (q1 - q0);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    // Rows are independent: four rows' loads are issued before the first tanh so their latencies
    // overlap (the per-row chain src_row -> lin row would otherwise serialise the whole graph).
    auto row_of = [&](int t) -> long { return t < np_ ? (long)(p0 + t) : n_clicks + (long)(q0 + t - np_); };
    auto load_row = [&](int t, float (&v)[4], long& e) {
        e = row_of(t);
        const float* lin = (t < np_ ? lin_p : lin_q) + (long)src_row[e] * ld_lin;
        const float* pe = pos_emb + (long)pos_id[e] * P;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c4 + u;
            v[u] = c < Dl ? lin[c] : pe[c - Dl];
        }
    };
    auto finish_row = [&](const float (&v)[4], long e) {
        const float4 o = make_float4(tanhf(v[0]), tanhf(v[1]), tanhf(v[2]), tanhf(v[3]));
        *reinterpret_cast<float4*>(node + e * ld_node + c4) = o;
        m.x += o.x; m.y += o.y; m.z += o.z; m.w += o.w;
    };
    int t = 0;
    for (; t + 4 <= cnt; t += 4) {
        float v0[4], v1[4], v2[4], v3[4];
        long e0, e1, e2, e3;
        load_row(t, v0, e0); load_row(t + 1, v1, e1); load_row(t + 2, v2, e2); load_row(t + 3, v3, e3);
        finish_row(v0, e0); finish_row(v1, e1); finish_row(v2, e2); finish_row(v3, e3);
    }
    for (; t < cnt; ++t) {
        float v0[4];
        long e0;
        load_row(t, v0, e0);
        finish_row(v0, e0);
    }
    const float inv = 1.f / (float)(cnt > 0 ? cnt : 1);
    *reinterpret_cast<float4*>(coarse + g * ld_coarse + c4) = make_float4(m.x * inv, m.y * inv, m.z * inv, m.w * inv);
}

// Second half (model/gnn.py:212-217): att_e = watt . sigmoid(a[e] + b[g]);  out[g] = mean_e(node[e] * att_e);
// normalize != 0 additionally applies the reference's `normalize` (util_amazon_filtered.py:28-31,
// x / sqrt(max(sum x^2, eps))) to the row, saving a pass over the session vectors.
template <int LPR>
__global__ __launch_bounds__(256) void k_pool_attention(const float* __restrict__ node, long ld_node,
                                                        const float* __restrict__ Aa, long ld_a,
                                                        const float* __restrict__ Bc, long ld_b,
                                                        const float* __restrict__ watt, const int* __restrict__ pptr,
                                                        const int* __restrict__ qptr, long n_clicks, long n_graphs,
                                                        int D, int normalize, float eps, int reduce_sum,
                                                        float* __restrict__ out, long ld_out) {
    const int sub = threadIdx.x % LPR;
    const long g = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const int c4 = sub * 4;
    const bool live = g < n_graphs && c4 < D;                   // dead lanes still take part in the shuffles
    int p0 = 0, p1 = 0, q0 = 0, q1 = 0;
    if (g < n_graphs) { p0 = pptr[g]; p1 = pptr[g + 1]; q0 = qptr[g]; q1 = qptr[g + 1]; }
    const int cnt = (p1 - p0) + (q1 - q0);
    float4 w4 = make_float4(0.f, 0.f, 0.f, 0.f), b4 = w4, acc = w4;
    if (live) { w4 = *reinterpret_cast<const float4*>(watt + c4); b4 = *reinterpret_cast<const float4*>(Bc + g * ld_b + c4); }
    auto row_of = [&](int t) -> long { return t < (p1 - p0) ? (long)(p0 + t) : n_clicks + (long)(q0 + t - (p1 - p0)); };
    auto load_row = [&](int t, float4& a, float4& v) {
        a = make_float4(0.f, 0.f, 0.f, 0.f); v = a;
        if (live && t < cnt) {
            const long e = row_of(t);
            a = *reinterpret_cast<const float4*>(Aa + e * ld_a + c4);
            v = *reinterpret_cast<const float4*>(node + e * ld_node + c4);
        }
    };
    auto finish_row = [&](const float4& a, const float4& v) {      // every lane of the group takes part in the shuffles
        const float part = live ? w4.x * sigmoidf_(a.x + b4.x) + w4.y * sigmoidf_(a.y + b4.y) + w4.z * sigmoidf_(a.z + b4.z) +
                                      w4.w * sigmoidf_(a.w + b4.w) : 0.f;
        acc = f4_fma(group_sum<LPR>(part), v, acc);
    };
    // cnt is uniform inside a lane group but differs between the groups of a wave: pad to the
    // wave-wide maximum so the shuffles stay convergent; padded rows load nothing and add 0.
    int cmax = cnt;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cmax = max(cmax, __shfl_xor(cmax, o));
    for (int t = 0; t < cmax; t += 4) {                             // four rows' loads in flight
        float4 a0, v0, a1, v1, a2, v2, a3, v3;
        load_row(t, a0, v0); load_row(t + 1, a1, v1); load_row(t + 2, a2, v2); load_row(t + 3, a3, v3);
        finish_row(a0, v0); finish_row(a1, v1); finish_row(a2, v2); finish_row(a3, v3);
    }
    const float inv = reduce_sum ? 1.f : 1.f / (float)(cnt > 0 ? cnt : 1);       // sum: SRGNN_Pooling's global_add_pool
    acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
    if (normalize) {
        const float ss = group_sum<LPR>(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w);
        const float den = sqrtf(fmaxf(ss, eps));
        acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den;
    }
    if (live) *reinterpret_cast<float4*>(out + g * ld_out + c4) = acc;
}

// PositionalAttentionPooling without materialising the expanded rows (3 launches instead of 4).
// An expanded row e is [tanh(lin[src(e)]) ; tanh(pos_emb[pid(e)])]: every LINEAR map of it splits into
// a per-NODE part and a per-POSITION table entry,
//     node_emb_lin(row e)   = A1[src(e)] + A2tab[pid(e)]      A1 = T Wn[:, :Dl]^T,  A2tab = tanh(P) Wn[:, Dl:]^T + bn
//     coarse_rep_lin(row e) = C1[src(e)] + C2tab[pid(e)]      C1 = T Wc[:, :Dl]^T,  C2tab = tanh(P) Wc[:, Dl:]^T
// with T = tanh(lin) per node (GEMM epilogue).  coarse_rep_lin of the graph MEAN is the mean of the
// rows' images, so one lane group per graph needs two passes over its rows and no [n_exp, D] buffers:
//   pass 1: bc = mean_e(C1[src] + C2tab[pid])
//   pass 2: att_e = watt . sigmoid(A1[src] + A2tab[pid] + bc);  out = mean_e(row_e * att_e)  (+ normalise)
// T / AC rows: products [0, Np), queries [Np, Np + Nq).  AC = [A1 | C1], 2D wide.
// One WAVE per graph: LPR lanes own the float4 columns of a row, the wave's 64 / LPR row slots take
// rows slot, slot + RS, ...; the (row -> node, position) indices of the whole graph are loaded once,
// one row per lane, and broadcast with shuffles, so both passes issue their gathers without a
// dependent index load in front.
template <int LPR>
__global__ __launch_bounds__(256) void k_pool_attention_tab(const float* __restrict__ T, long ld_t, const float* __restrict__ AC,
                                                            long ld_ac, const float* __restrict__ tanhpos,
                                                            const float* __restrict__ A2tab, const float* __restrict__ C2tab,
                                                            const float* __restrict__ watt, const int* __restrict__ src_row,
                                                            const int* __restrict__ pos_id, const int* __restrict__ pptr,
                                                            const int* __restrict__ qptr, long n_clicks, long Np,
                                                            long n_graphs, int Dl, int P, int normalize, float eps,
                                                            float* __restrict__ out, long ld_out) {
    constexpr int RS = 64 / LPR;                                 // row slots per wave
    const int lane = threadIdx.x & 63;
    const int sub = lane % LPR, slot = lane / LPR;
    const long g = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (g >= n_graphs) return;                                   // whole wave
    const int D = Dl + P, c4 = sub * 4;
    const bool colok = c4 < D;
    const int p0 = pptr[g], p1 = pptr[g + 1], q0 = qptr[g], q1 = qptr[g + 1];
    const int np_ = p1 - p0, cnt = np_ + (q1 - q0);
    const float inv = 1.f / (float)(cnt > 0 ? cnt : 1);
    float4 bc = make_float4(0.f, 0.f, 0.f, 0.f), acc = bc, w4 = bc;
    if (colok) w4 = *reinterpret_cast<const float4*>(watt + c4);
    for (int base = 0; base < cnt; base += 64) {                 // graphs longer than 64 rows: chunks (bc needs all rows first)
        const int t_l = base + lane;
        int my_node = 0, my_pid = 0;
        if (t_l < cnt) {
            const long e = t_l < np_ ? (long)(p0 + t_l) : n_clicks + (long)(q0 + t_l - np_);
            my_node = (int)((t_l < np_ ? 0 : Np) + src_row[e]);
            my_pid = pos_id[e];
        }
        const int nrow = min(64, cnt - base);
        for (int r0 = 0; r0 < nrow; r0 += RS) {                  // pass 1 (this chunk): sum of C1[node] + C2tab[pid]
            const int r = r0 + slot;
            const int node = __shfl(my_node, r & 63), pid = __shfl(my_pid, r & 63);
            if (r < nrow && colok) {
                const float4 v = *reinterpret_cast<const float4*>(AC + (long)node * ld_ac + D + c4);
                const float4 w = *reinterpret_cast<const float4*>(C2tab + (long)pid * D + c4);
                bc.x += v.x + w.x; bc.y += v.y + w.y; bc.z += v.z + w.z; bc.w += v.w + w.w;
            }
        }
    }
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {                         // combine the row slots
        bc.x += __shfl_xor(bc.x, o); bc.y += __shfl_xor(bc.y, o); bc.z += __shfl_xor(bc.z, o); bc.w += __shfl_xor(bc.w, o);
    }
    bc.x *= inv; bc.y *= inv; bc.z *= inv; bc.w *= inv;
    for (int base = 0; base < cnt; base += 64) {                 // pass 2: attention-weighted sum
        const int t_l = base + lane;
        int my_node = 0, my_pid = 0;
        if (t_l < cnt) {
            const long e = t_l < np_ ? (long)(p0 + t_l) : n_clicks + (long)(q0 + t_l - np_);
            my_node = (int)((t_l < np_ ? 0 : Np) + src_row[e]);
            my_pid = pos_id[e];
        }
        const int nrow = min(64, cnt - base);
        for (int r0 = 0; r0 < nrow; r0 += RS) {
            const int r = r0 + slot;
            const int node = __shfl(my_node, r & 63), pid = __shfl(my_pid, r & 63);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            float part = 0.f;
            if (r < nrow && colok) {
                const float4 a1 = *reinterpret_cast<const float4*>(AC + (long)node * ld_ac + c4);
                const float4 a2 = *reinterpret_cast<const float4*>(A2tab + (long)pid * D + c4);
                float xv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c4 + j;
                    xv[j] = c < Dl ? T[(long)node * ld_t + c] : tanhpos[(long)pid * P + (c - Dl)];
                }
                x = make_float4(xv[0], xv[1], xv[2], xv[3]);
                part = w4.x * sigmoidf_(a1.x + a2.x + bc.x) + w4.y * sigmoidf_(a1.y + a2.y + bc.y) +
                       w4.z * sigmoidf_(a1.z + a2.z + bc.z) + w4.w * sigmoidf_(a1.w + a2.w + bc.w);
            }
            acc = f4_fma(group_sum<LPR>(part), x, acc);
        }
    }
#pragma unroll
    for (int o = LPR; o < 64; o <<= 1) {
        acc.x += __shfl_xor(acc.x, o); acc.y += __shfl_xor(acc.y, o); acc.z += __shfl_xor(acc.z, o); acc.w += __shfl_xor(acc.w, o);
    }
    acc.x *= inv; acc.y *= inv; acc.z *= inv; acc.w *= inv;
    if (normalize) {
        const float ss = group_sum<LPR>(acc.x * acc.x + acc.y * acc.y + acc.z * acc.z + acc.w * acc.w);
        const float den = sqrtf(fmaxf(ss, eps));
        acc.x /= den; acc.y /= den; acc.z /= den; acc.w /= den;
    }
    if (slot == 0 && colok) *reinterpret_cast<float4*>(out + g * ld_out + c4) = acc;
}

// ------------------------------------------------------------------------------ host launchers
// (none of these kernels grid-strides: every lane group, or wave, gets exactly one row -- GRID_ALL)
extern "C" int sss_hetero_layer_update(const sss_layer_args* args, void* stream) {
    if (!args) { set_error("hetero_layer_update: null args"); return SSS_EINVAL; }
    const sss_layer_args& a = *args;
    if (a.h <= 0 || a.h % 4 || a.h > 256 || a.np < 0 || a.nq < 0 || a.d_x > a.h || a.ld_yp % 4 || a.ld_yq % 4 || a.ld_out_p % 4 ||
        a.ld_out_q % 4 || (a.d_x >= 4 && a.ld_xin % 4) || a.ld_yp < 7 * a.h + 2 || a.ld_yq < a.h + 2) {
        set_error("layer_update: need h %% 4 == 0, h <= 256, d_x <= h, 16-byte aligned row strides, ldyp >= 7h+2, ldyq >= h+2");
        return SSS_EINVAL;
    }
    if ((a.x0_p && a.ld_x0_p % 4) || (a.x0_q && (!a.xq_table || a.ld_xq % 4 || a.ld_x0_q % 4))) {
        set_error("layer_update: x0_p / x0_q need 16-byte aligned row strides, x0_q needs xq_table");
        return SSS_EINVAL;
    }
    const long total = a.np + a.nq;
    if (total == 0) return SSS_OK;
    SSS_LPR_SWITCH(lanes_for(a.h), hipLaunchKernelGGL(k_layer_update<L>, dim3(grid_blocks(total, 256 / L, GRID_ALL)), dim3(256), 0,
                                                      static_cast<hipStream_t>(stream), a));
    return check_launch("k_layer_update");
}

extern "C" int sss_pool_expand_mean(const float* lin_p, const float* lin_q, int64_t ld_lin, const int32_t* src_row,
                                    const int32_t* pos_id, const int32_t* pptr, const int32_t* qptr, int64_t n_clicks, int64_t n_graphs,
                                    int d_lin, int p, const float* pos_emb, float* node, int64_t ld_node, float* coarse,
                                    int64_t ld_coarse, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int D = d_lin + p;
    if (n_graphs < 0 || d_lin <= 0 || p < 0 || D % 4 || D > 256 || ld_node % 4 || ld_node < D || ld_coarse % 4 || ld_coarse < D) {
        set_error("pool_expand_mean: need (Dl + P) %% 4 == 0, <= 256, 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_graphs == 0) return SSS_OK;
    SSS_LPR_SWITCH(lanes_for(D), hipLaunchKernelGGL(k_pool_expand_mean<L>, dim3(grid_blocks(n_graphs, 256 / L, GRID_ALL)), dim3(256), 0,
                                                    st, lin_p, lin_q, ld_lin, src_row, pos_id, pptr, qptr, n_clicks, n_graphs, d_lin, p,
                                                    pos_emb, node, ld_node, coarse, ld_coarse));
    return check_launch("k_pool_expand_mean");
}

extern "C" int sss_pool_attention(const float* node, int64_t ld_node, const float* a, int64_t ld_a, const float* b, int64_t ld_b,
                                  const float* watt, const int32_t* pptr, const int32_t* qptr, int64_t n_clicks, int64_t n_graphs,
                                  int d, int normalize, float eps, int reduce_sum, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_graphs < 0 || d <= 0 || d % 4 || ld_node % 4 || ld_a % 4 || ld_b % 4 || ld_out % 4 || ld_out < d) {
        set_error("pool_attention: need D %% 4 == 0, 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_graphs == 0) return SSS_OK;
    if (d > 256) {
        // rows wider than one float4 column per lane (the reference's gnn_nout = 800, config.py:16): the column-chunked
        // sweep of k_segment_pool (gnn.hip), which computes a node's attention weight once for all of a lane's columns
        const int rc = launch_segment_pool(node, ld_node, pptr, qptr, n_clicks, n_graphs, d, a, ld_a, b, ld_b, watt, out, ld_out,
                                           reduce_sum, st);
        if (rc || !normalize) return rc;
        return sss_normalize_rows(out, n_graphs, d, ld_out, eps, 0, st);
    }
    SSS_LPR_SWITCH(lanes_for(d), hipLaunchKernelGGL(k_pool_attention<L>, dim3(grid_blocks(n_graphs, 256 / L, GRID_ALL)), dim3(256), 0, st,
                                                    node, ld_node, a, ld_a, b, ld_b, watt, pptr, qptr, n_clicks, n_graphs, d, normalize,
                                                    eps, reduce_sum, out, ld_out));
    return check_launch("k_pool_attention");
}

extern "C" int sss_pool_attention_tab(const float* t, int64_t ld_t, const float* ac, int64_t ld_ac, const float* tanhpos,
                                      const float* a2tab, const float* c2tab, const float* watt, const int32_t* src_row,
                                      const int32_t* pos_id, const int32_t* pptr, const int32_t* qptr, int64_t n_clicks, int64_t np,
                                      int64_t n_graphs, int d_lin, int p, int normalize, float eps, float* out, int64_t ld_out,
                                      void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int D = d_lin + p;
    if (n_graphs < 0 || d_lin <= 0 || p < 0 || D % 4 || D > 256 || ld_t < d_lin || ld_ac % 4 || ld_ac < 2 * D || ld_out % 4 || ld_out < D) {
        set_error("pool_attention_tab: need (Dl + P) %% 4 == 0, <= 256, ld_ac >= 2 (Dl + P), 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n_graphs == 0) return SSS_OK;
    // one wave per graph, four a workgroup
    SSS_LPR_SWITCH(lanes_for(D), hipLaunchKernelGGL(k_pool_attention_tab<L>, dim3(grid_blocks(n_graphs, 4, GRID_ALL)), dim3(256), 0, st, t,
                                                    ld_t, ac, ld_ac, tanhpos, a2tab, c2tab, watt, src_row, pos_id, pptr, qptr, n_clicks,
                                                    np, n_graphs, d_lin, p, normalize, eps, out, ld_out));
    return check_launch("k_pool_attention_tab");
}

}  // namespace sss
