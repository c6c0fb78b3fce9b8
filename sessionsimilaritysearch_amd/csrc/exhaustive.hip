// Exhaustive exact search: canonical float64 scores of selected queries against EVERY corpus
// row, then an exact top-k.  This is the correctness backstop behind the fused scans (queries
// whose fused result could not be proven exact, tiny corpora, k larger than the fused path,
// the IndexFlatL2 metric of reference test_amazon_filterd.py:215-217, any d % 4 == 0 such as
// the reference's D = 1600).  O(n d) scoring here, then the exact top-k of the score matrix
// (topk_scores.hip); the scorers also feed the exhaustive range search (range_exhaustive.hip).
// DESIGN.md "exactness".
#include "scan.h"

namespace sss {

constexpr int EX_ROWS = 64;   // rows per wave pass
constexpr int EX_KC = 128;    // k-chunk staged in LDS
constexpr int EX_LD = EX_KC + 4;

// scores[f][row] = float32( sum_k q[qsel[f]][k] * c[row][k] ) accumulated sequentially in
// float64 (metric 0), or sum_k (q_k - c_k)^2 with one rounding per multiply and per add (1).
// DT_BF16 / DT_H16 / DT_I8: q and c hold bf16 / float16 / int8; every element converts exactly to float32 on the way into
// LDS (int8: every partial sum of either metric is an integer below 2^53, so the chain rounds nowhere).
template <int DT>
__global__ __launch_bounds__(64) void k_exact_scores(const void* __restrict__ Qv,
                                                     const int* __restrict__ qsel,
                                                     const void* __restrict__ Cv, long n, int d,
                                                     int metric, float* __restrict__ scores) {
    __shared__ __attribute__((aligned(16))) float tile[EX_ROWS * EX_LD];
    __shared__ __attribute__((aligned(16))) float qs[EX_KC];
    constexpr int EB = Elem<DT>::bytes;               // bytes per element
    constexpr int EPV = Elem<DT>::per_chunk;          // elements per 16-byte load
    const int lane = threadIdx.x;
    const int f = blockIdx.y;
    const char* C = reinterpret_cast<const char*>(Cv);
    const char* q = reinterpret_cast<const char*>(Qv) + (size_t)qsel[f] * d * EB;
    for (long row0 = (long)blockIdx.x * EX_ROWS; row0 < n; row0 += (long)gridDim.x * EX_ROWS) {
        double acc = 0.0;
        for (int k0 = 0; k0 < d; k0 += EX_KC) {
            const int kc = d - k0 < EX_KC ? d - k0 : EX_KC;   // multiple of EPV
            const int nv = kc / EPV;
            __syncthreads();
            for (int i = lane; i < EX_ROWS * nv; i += 64) {
                const int rr = i / nv, cc = i % nv;
                long grow = row0 + rr;
                if (grow > n - 1) grow = n - 1;
                const f32x4 v = *reinterpret_cast<const f32x4*>(C + ((size_t)grow * d + k0) * EB + cc * 16);
#pragma unroll
                for (int e = 0; e < EPV; ++e) tile[rr * EX_LD + cc * EPV + e] = Elem<DT>::to_f32(&v, e);
            }
            for (int i = lane; i < kc; i += 64) qs[i] = Elem<DT>::to_f32(q, k0 + i);
            __syncthreads();
            const float* mine = &tile[lane * EX_LD];
            if (metric == 0) {
                for (int kk = 0; kk < kc; ++kk) acc += (double)qs[kk] * (double)mine[kk];
            } else {
                for (int kk = 0; kk < kc; ++kk) acc = l2_chain_step(acc, (double)qs[kk], (double)mine[kk]);
            }
        }
        if (row0 + lane < n) scores[(size_t)f * n + row0 + lane] = (float)acc;
    }
}

// Fast scorer for the fused kernel's shapes (d = 64 / 128 / 256 elements per row): a lane keeps
// ONE corpus row in registers and walks all selected queries, so the corpus is read once however
// many queries need the backstop (k_exact_scores above re-reads it per query).  The query elements are
// wave-uniform: they come in through the scalar cache (s_load) and enter the FMAs as SGPR operands --
// no LDS, no barrier.  Same canonical score: sequential float64 sum.
// lb (optional, one float per selected query): a LOWER bound of the query's k-th best score (the fused
// path's k-th re-scored candidate).  A cheap float32 pass first bounds every row's score from above
// (float32 fma chain: error <= d 2^-24 |q||c| + d 2^-150); rows that provably stay below lb -- almost all of them --
// skip the float64 chain and get -FLT_MAX, which the selection ignores.
template <int DT>
__device__ __forceinline__ float q_elem(const void* qrow, int kx) {        // element kx of a (wave-uniform) query row: its 32-bit word
    constexpr int PW = 4 / Elem<DT>::bytes;
    return Elem<DT>::from_word(reinterpret_cast<const unsigned*>(qrow)[kx / PW], kx % PW);
}

template <int D, int DT>
__global__ __launch_bounds__(256) void k_exact_scores_rows(const void* __restrict__ Qv, const int* __restrict__ qsel, int nsel,
                                                           const void* __restrict__ Cv, long n, float* __restrict__ scores,
                                                           const float* __restrict__ lb, int lb_by_row) {
    constexpr int QB = 1024;                           // queries whose norms are kept in LDS at a time
    __shared__ double qn[QB];
    constexpr int EB = Elem<DT>::bytes, EPV = Elem<DT>::per_chunk, PW = EPV / 4;   // PW: elements per 32-bit word
    const char* C = reinterpret_cast<const char*>(Cv);
    const char* Q = reinterpret_cast<const char*>(Qv);
    const long row = (long)blockIdx.x * 256 + threadIdx.x;
    const long rl = row < n ? row : n - 1;
    float r[D];
#pragma unroll
    for (int v = 0; v < D / EPV; ++v) {
        const u32x4 c4 = *reinterpret_cast<const u32x4*>(C + ((size_t)rl * D + v * EPV) * EB);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int j = 0; j < PW; ++j) r[EPV * v + PW * e + j] = Elem<DT>::from_word(c4[e], j);
    }
    // norms for the pre-test's margin in float64 (squares of float32 values are exact there): a float32 sum of squares
    // is 0 for rows below ~1e-19 and inf above ~1.8e19, which would shrink the margin to nothing / widen it to everything
    double rnorm = 0.0;
    if (lb) {
#pragma unroll
        for (int kx = 0; kx < D; ++kx) rnorm += (double)r[kx] * (double)r[kx];
        rnorm = sqrt(rnorm) * 1.0001;
    }
    for (int f0 = 0; f0 < nsel; f0 += QB) {
        const int nf = nsel - f0 < QB ? nsel - f0 : QB;
        if (lb) {                                          // query norms of this block (for the pre-test's error margin)
            __syncthreads();
            for (int t = threadIdx.x; t < nf; t += 256) {
                const char* qrow = Q + (size_t)qsel[f0 + t] * D * EB;
                double s2 = 0.0;
                for (int kx = 0; kx < D; ++kx) { const double v = q_elem<DT>(qrow, kx); s2 += v * v; }
                qn[t] = sqrt(s2) * 1.0001;
            }
            __syncthreads();
        }
        for (int f = 0; f < nf; ++f) {
            const char* qrow = Q + (size_t)qsel[f0 + f] * D * EB;      // wave-uniform address: scalar loads
            bool need = true;
            if (lb) {                                      // float32 upper bound first
                float s0 = 0.f;
#pragma unroll
                for (int kx = 0; kx < D; ++kx) s0 = fmaf(q_elem<DT>(qrow, kx), r[kx], s0);
                // margin in float64: the chain's relative error, its gradual underflow (D roundings of at most 2^-150 each
                // below FLT_MIN) and one float32 ulp of l0 (2^-149 absolute in the subnormal range)
                const float l0 = lb[lb_by_row ? qsel[f0 + f] : f0 + f];    // (per selected query, or per query row)
                need = !((double)s0 + (double)D * 6.3e-8 * rnorm * qn[f] + ULP32_REL * fabs((double)l0) + (D + 8) * 1.4012984643248171e-45 <
                         (double)l0);                      // (NaN anywhere: keep the row)
            }
            double acc = 0.0;
            if (need) {
#pragma unroll
                for (int kx = 0; kx < D; ++kx) acc += (double)q_elem<DT>(qrow, kx) * (double)r[kx];
            }
            if (row < n) scores[(size_t)(f0 + f) * n + row] = need ? (float)acc : -3.4028234663852886e38f;
        }
    }
}

// (scan.h)
int launch_exact_scores(const void* q, const int* qsel, long nsel, const void* c, long n, int d, int dtype, int metric, float* scores,
                        const float* lb, int lb_by_row, hipStream_t st) {
    long gx = (n + EX_ROWS - 1) / EX_ROWS;
    if (gx > 8192) gx = 8192;
    const unsigned rb = (unsigned)((n + 255) / 256);
    // the row-resident form: inner product, rows of 256 / 512 bytes (float32: 1024 as well); none for int8 rows, whose
    // every shape ignores the bound
    const bool known = with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        [[maybe_unused]] auto rows = [&](auto dd) {
            hipLaunchKernelGGL((k_exact_scores_rows<decltype(dd)::value, DT>), dim3(rb), dim3(256), 0, st, q, qsel, (int)nsel, c, n, scores, lb, lb_by_row);
        };
        if constexpr (DT == DT_F32) {
            if (metric == 0 && d == 64) return rows(std::integral_constant<int, 64>());
        }
        if constexpr (DT != DT_I8) {
            if (metric == 0 && d == 128) return rows(std::integral_constant<int, 128>());
            if (metric == 0 && d == 256) return rows(std::integral_constant<int, 256>());
        }
        hipLaunchKernelGGL(k_exact_scores<DT>, dim3((unsigned)gx, (unsigned)nsel), dim3(64), 0, st, q, qsel, c, n, d, metric, scores);
    });
    if (!known) { set_error("exact scores: dtype %d is not a corpus dtype", dtype); return SSS_EINVAL; }
    return check_launch("k_exact_scores");
}

extern "C" size_t sss_ip_topk_exhaustive_workspace_bytes(int64_t nsel, int64_t n) {
    return score_matrix_bytes(nsel, n) + 256 + topk_of_scores_bytes(nsel, n);
}

// sss_ip_topk_exhaustive and sss_ip_topk_exhaustive_lb below are the two views of this one
static int ip_topk_exhaustive(const void* q, const int* qsel, long nsel, const void* c, long n, int d,
                              int k, int dtype, long id_offset, int metric, const float* lower_bound, float* D_out, long* I_out,
                              void* ws, size_t ws_bytes, hipStream_t st) {
    if (nsel <= 0 || n <= 0 || k <= 0 || d <= 0 || !corpus_dtype_ok(dtype) ||
        d % elems_per_chunk(dtype) || (metric != 0 && metric != 1)) {
        set_error("ip_topk_exhaustive: need nsel, n, k > 0, %s, metric in {0,1}", row_align_text());
        return SSS_EINVAL;
    }
    if (n >= (1L << 31) || nsel > 65535 || k > RS_MAX_K) { set_error("ip_topk_exhaustive: n < 2^31, nsel <= 65535, k <= 1024"); return SSS_EINVAL; }
    if (ws_bytes < sss_ip_topk_exhaustive_workspace_bytes(nsel, n)) {
        set_error("ip_topk_exhaustive: workspace too small");
        return SSS_EWORKSPACE;
    }
    float* scores = reinterpret_cast<float*>(ws);
    int rc = launch_exact_scores(q, qsel, nsel, c, n, d, dtype, metric, scores, lower_bound, 0, st);
    if (rc) return rc;
    return topk_of_scores(scores, qsel, nsel, n, k, id_offset, metric, D_out, I_out, reinterpret_cast<char*>(ws) + score_matrix_bytes(nsel, n), st);
}

extern "C" int sss_ip_topk_exhaustive(const void* q, const int32_t* qsel, int64_t nsel, const void* corpus, int64_t n, int d, int k, int dtype,
                                      int64_t id_offset, int metric, float* D_out, int64_t* I_out, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    return ip_topk_exhaustive(q, qsel, nsel, corpus, n, d, k, dtype, id_offset, metric, nullptr, D_out, I_out, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

extern "C" int sss_ip_topk_exhaustive_lb(const void* q, const int32_t* qsel, int64_t nsel, const void* corpus, int64_t n, int d, int k,
                                         int dtype, int64_t id_offset, const float* lower_bound, float* D_out, int64_t* I_out,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    return ip_topk_exhaustive(q, qsel, nsel, corpus, n, d, k, dtype, id_offset, 0, lower_bound, D_out, I_out, workspace, workspace_bytes,
                              static_cast<hipStream_t>(stream));
}

}  // namespace sss
