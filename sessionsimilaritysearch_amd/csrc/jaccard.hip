// Ground truth over the whole corpus: the item-set Jaccard of a query against every corpus row (the 'all_jaccard' /
// 'cur_jaccard' kinds of the reference's get_score, fine_tune_ours.py:42-55), its exact top-k, and the band counts / first
// rows of the fine-tuning triple mining (fine_tune_ours.py:187-235).  C ABI and THE CONTRACT: include/sss_jaccard.h;
// measurements: DESIGN.md 5.7.
//
// Both kernels are k_sparse_scores' walk (sparse.hip) with an integer accumulator: a thread owns a corpus row, the first
// JC_D items of the row sit in the thread's own LDS column ([entry][thread]: the bank is the thread's, whatever entry each
// lane is at), a wave holding a longer row walks global memory instead -- the choice is per wave, so each loop has one
// address space -- and the query's items are wave-uniform loads.
//
//   k_jaccard_scores    writes float32(inter / uni) for every pair and the identity query selection; topk_of_scores
//                       (exhaustive.hip, metric 0) is the unchanged tail
//   k_jaccard_bands     no matrix: per query one ballot per band over the wave (the popcount is the count; the lowest set
//                       lane is the lowest row, rows ascend with the lane); the four waves' words of JC_QRUN queries meet in
//                       LDS and one thread per (query, band) adds the workgroup's total with integer atomics
#include <math.h>

#include "scan.h"

namespace sss {

constexpr int JC_ROWS = 256;
// Items only, no weights: the 32 KiB that hold 16 (item, weight) entries per row in k_sparse_scores hold 32 items here.
// Every row session_vectors builds from the benchmark corpora (at most 19 actions) and all but the longest real sessions
// then take the LDS form; 64 would cover the builder's limit but leaves 2 workgroups a CU (64 KiB each) where 32 leaves 4.
constexpr int JC_D = 32;
constexpr int JC_QRUN = 32;           // queries between two flushes of k_jaccard_bands: 256 threads = 32 queries x 8 bands
constexpr int JC_MAX_EDGES = 7;
constexpr int JC_BANDS = JC_MAX_EDGES + 1;
constexpr int JC_MAX_K = 1024;        // k_topk_radix's RS_MAX_K

// The two measured experiments of DESIGN.md 5.7, kept as build switches so that either can be timed again:
//   JC_SIGNATURE  the 64-bit item-hash signature pre-test (a pair whose signatures do not meet has inter = 0 unwalked)
//   JC_STAGE      per-workgroup band totals staged in LDS for JC_QRUN queries (0: every wave adds its own to global memory)
#ifndef JC_SIGNATURE
#define JC_SIGNATURE 0
#endif
#ifndef JC_STAGE
#define JC_STAGE 1
#endif

struct JcEdges { double e[JC_MAX_EDGES]; };     // unused edges are +inf: no ratio reaches them

__device__ __forceinline__ int jc_len(long a, long b) {
    const long l = b - a;
    return l < 0 ? 0 : l > 0x7fffffffL ? 0x7fffffff : (int)l;
}

__device__ __forceinline__ unsigned long long jc_bit(int item) { return 1ull << (((unsigned)item * 0x9E3779B1u) >> 26); }

struct JcRow {
    long r0;                  // the row's first entry in citems
    int lr;                   // its length (0 beyond the corpus)
    bool wave_long;           // some row of this wave is longer than its LDS column
    unsigned long long sig;   // JC_SIGNATURE: OR of jc_bit over the row
};

// The thread's row: its first JC_D items into the thread's LDS column (read back by this thread alone: no barrier).
__device__ __forceinline__ JcRow jc_stage(const long* __restrict__ cptr, const int* __restrict__ citems, long row, long n, int* r_it,
                                          int tid) {
    JcRow R{0, 0, false, 0ull};
    if (row < n) {
        R.r0 = cptr[row];
        R.lr = jc_len(R.r0, cptr[row + 1]);
    }
    for (int j = 0; j < JC_D && j < R.lr; ++j) {
        const int it = citems[R.r0 + j];
        r_it[j * JC_ROWS + tid] = it;
#if JC_SIGNATURE
        R.sig |= jc_bit(it);
#endif
    }
#if JC_SIGNATURE
    for (int j = JC_D; j < R.lr; ++j) R.sig |= jc_bit(citems[R.r0 + j]);
#endif
    R.wave_long = __builtin_amdgcn_ballot_w64(R.lr > JC_D) != 0ull;
    return R;
}

#if JC_SIGNATURE
// Signatures of the queries [f0, fe) into s_qsig, one thread each; the caller's barriers stand on both sides.
__device__ __forceinline__ void jc_query_sigs(const long* __restrict__ qptr, const int* __restrict__ qitems, int f0, int fe, int tid,
                                              unsigned long long* s_qsig) {
    if (tid < fe - f0) {
        const long q0 = qptr[f0 + tid];
        const int ql = jc_len(q0, qptr[f0 + tid + 1]);
        unsigned long long s = 0ull;
        for (int p = 0; p < ql; ++p) s |= jc_bit(qitems[q0 + p]);
        s_qsig[tid] = s;
    }
}
#endif

// |Q & C| for the thread's row of `lr` items (`first` = its first item, or the sentinel): each lane advances through its row
// as the query's items ascend.  Item ids are below 2^31 - 1, the sentinel.
template <class ItemAt>
__device__ __forceinline__ int jc_inter(const int* __restrict__ qitems, long q0, long q1, int lr, int first, ItemAt item_at) {
    int j = 0, cur = first, acc = 0;
    for (long p = q0; p < q1; ++p) {
        const int qi = qitems[p];
        while (cur < qi) {
            ++j;
            cur = j < lr ? item_at(j) : 0x7fffffff;
        }
        if (cur == qi && j < lr) ++acc;
    }
    return acc;
}

// inter of (query f, the thread's row); with JC_SIGNATURE a wave none of whose rows can meet the query skips the walk, and
// in a wave that walks the rows that cannot meet it take no step.
template <class ItemAt>
__device__ __forceinline__ int jc_pair(const int* __restrict__ qitems, long q0, long q1, const JcRow& R, int first,
                                       unsigned long long qsig, ItemAt item_at) {
#if JC_SIGNATURE
    const bool meet = (R.sig & qsig) != 0ull;
    if (__builtin_amdgcn_ballot_w64(meet) == 0ull) return 0;
    return jc_inter(qitems, q0, q1, meet ? R.lr : 0, meet ? first : 0x7fffffff, item_at);
#else
    return jc_inter(qitems, q0, q1, R.lr, first, item_at);
#endif
}

// grid (row blocks, query ranges); block (0, y) also writes the identity query selection the top-k reads.
__global__ __launch_bounds__(JC_ROWS) void k_jaccard_scores(const long* __restrict__ qptr, const int* __restrict__ qitems, int nq,
                                                            int q_per, const long* __restrict__ cptr, const int* __restrict__ citems,
                                                            long n, float* __restrict__ scores, int* __restrict__ qsel) {
    __shared__ int r_it[JC_D * JC_ROWS];
#if JC_SIGNATURE
    __shared__ unsigned long long s_qsig[JC_QRUN];
#endif
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * JC_ROWS + tid;
    const JcRow R = jc_stage(cptr, citems, row, n, r_it, tid);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    for (int f0 = f_lo; f0 < f_hi; f0 += JC_QRUN) {              // workgroup-uniform: the barriers below are met by all
        const int fe = f0 + JC_QRUN < f_hi ? f0 + JC_QRUN : f_hi;
#if JC_SIGNATURE
        __syncthreads();
        jc_query_sigs(qptr, qitems, f0, fe, tid, s_qsig);
        __syncthreads();
#endif
        auto run = [&](auto item_at) {
            const int first = R.lr > 0 ? item_at(0) : 0x7fffffff;
            for (int f = f0; f < fe; ++f) {
                if (blockIdx.x == 0 && tid == 0) qsel[f] = f;
                const long q0 = qptr[f], q1 = q0 + jc_len(q0, qptr[f + 1]);
#if JC_SIGNATURE
                const unsigned long long qs = s_qsig[f - f0];
#else
                const unsigned long long qs = 0ull;
#endif
                const int acc = jc_pair(qitems, q0, q1, R, first, qs, item_at);
                const long uni = (q1 - q0) + R.lr - acc;
                if (row < n) scores[(size_t)f * n + row] = uni ? (float)__ddiv_rn((double)acc, (double)uni) : 0.f;
            }
        };
        if (!R.wave_long)
            run([&](int j) { return r_it[j * JC_ROWS + tid]; });
        else
            run([&](int j) { return citems[R.r0 + j]; });
    }
}

// counts / first: [nq][nb] with nb = edges + 1, zeroed / set to all ones (int64 -1 = the largest unsigned value, so an
// unsigned atomicMin of row + id_offset >= 0 leaves -1 exactly where a band has no row) by the entry point.
__global__ __launch_bounds__(JC_ROWS) void k_jaccard_bands(const long* __restrict__ qptr, const int* __restrict__ qitems, int nq,
                                                           int q_per, const long* __restrict__ cptr, const int* __restrict__ citems,
                                                           long n, const JcEdges E, int nb, long id_offset,
                                                           unsigned long long* __restrict__ counts,
                                                           unsigned long long* __restrict__ first_out) {
    __shared__ int r_it[JC_D * JC_ROWS];
#if JC_SIGNATURE
    __shared__ unsigned long long s_qsig[JC_QRUN];
#endif
#if JC_STAGE
    __shared__ int s_tot[JC_ROWS / 64][JC_QRUN][JC_BANDS];       // (rows of the band in the wave) << 8 | its lowest lane; 0: none
#endif
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long row0 = (long)blockIdx.x * JC_ROWS, row = row0 + tid;
    const JcRow R = jc_stage(cptr, citems, row, n, r_it, tid);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    for (int f0 = f_lo; f0 < f_hi; f0 += JC_QRUN) {              // workgroup-uniform: the barriers below are met by all
        const int fe = f0 + JC_QRUN < f_hi ? f0 + JC_QRUN : f_hi;
#if JC_SIGNATURE
        __syncthreads();
        jc_query_sigs(qptr, qitems, f0, fe, tid, s_qsig);
        __syncthreads();
#endif
        auto run = [&](auto item_at) {
            const int first = R.lr > 0 ? item_at(0) : 0x7fffffff;
            for (int f = f0; f < fe; ++f) {
                const long q0 = qptr[f], q1 = q0 + jc_len(q0, qptr[f + 1]);
#if JC_SIGNATURE
                const unsigned long long qs = s_qsig[f - f0];
#else
                const unsigned long long qs = 0ull;
#endif
                const int acc = jc_pair(qitems, q0, q1, R, first, qs, item_at);
                const long uni = (q1 - q0) + R.lr - acc;
                const double s = uni ? __ddiv_rn((double)acc, (double)uni) : 0.0;
                int band = 0;
#pragma unroll
                for (int e = 0; e < JC_MAX_EDGES; ++e) band += s >= E.e[e] ? 1 : 0;
                int mine = 0;                                    // lane b: band b's word for this wave
                for (int b = 0; b < nb; ++b) {
                    const unsigned long long m = __builtin_amdgcn_ballot_w64(row < n && band == b);
                    if (lane == b && m) mine = (__builtin_popcountll(m) << 8) | __builtin_ctzll(m);
                }
#if JC_STAGE
                if (lane < JC_BANDS) s_tot[wv][f - f0][lane] = mine;
#else
                if (mine) {
                    const size_t at = (size_t)f * nb + lane;
                    atomicAdd(&counts[at], (unsigned long long)(mine >> 8));
                    atomicMin(&first_out[at], (unsigned long long)(row0 + wv * 64 + (mine & 255) + id_offset));
                }
#endif
            }
        };
        if (!R.wave_long)
            run([&](int j) { return r_it[j * JC_ROWS + tid]; });
        else
            run([&](int j) { return citems[R.r0 + j]; });
#if JC_STAGE
        __syncthreads();
        const int q = tid >> 3, b = tid & 7;                     // JC_ROWS = JC_QRUN * JC_BANDS: one thread per (query, band)
        if (f0 + q < fe && b < nb) {
            int cnt = 0, lo = -1;
            for (int w = 0; w < JC_ROWS / 64; ++w) {             // waves ascend with the rows: the first hit is the lowest
                const int t = s_tot[w][q][b];
                if (t) {
                    cnt += t >> 8;
                    if (lo < 0) lo = w * 64 + (t & 255);
                }
            }
            if (cnt) {
                const size_t at = (size_t)(f0 + q) * nb + b;
                atomicAdd(&counts[at], (unsigned long long)cnt);
                atomicMin(&first_out[at], (unsigned long long)(row0 + lo + id_offset));
            }
        }
        __syncthreads();
#endif
    }
}
static_assert(JC_ROWS == JC_QRUN * JC_BANDS, "the flush maps one thread to one (query, band)");

// ------------------------------------------------------------------------------ host launchers
static int jc_sets_ok(const char* what, const void* q_ptr, const void* q_items, long nq, const void* c_ptr, const void* c_items, long n) {
    if (nq <= 0 || nq > 65535 || n <= 0 || n >= (1L << 31)) {
        set_error("%s: need 0 < nq <= 65535, 0 < n < 2^31", what);
        return SSS_EINVAL;
    }
    if (!q_ptr || !q_items || !c_ptr || !c_items) {
        set_error("%s: a null pointer (both item sets are required)", what);
        return SSS_EINVAL;
    }
    return SSS_OK;
}

// grid of both kernels: a small corpus splits the queries too, ~1024 workgroups (as sss_sparse_topk)
static dim3 jc_grid(long nq, long n, int* q_per) {
    const long nbx = (n + JC_ROWS - 1) / JC_ROWS;
    long ny = (1024 + nbx - 1) / nbx;
    if (ny > nq) ny = nq;
    *q_per = (int)((nq + ny - 1) / ny);
    ny = (nq + *q_per - 1) / *q_per;
    return dim3((unsigned)nbx, (unsigned)ny);
}

// Workspace: scores f32 [nq][n] | (256-byte aligned) identity query selection i32 [nq] | (aligned) the top-k's tail.
static size_t jc_scores_bytes(long nq, long n) { return ((size_t)nq * n * 4 + 255) & ~(size_t)255; }
static size_t jc_qsel_bytes(long nq) { return ((size_t)nq * 4 + 255) & ~(size_t)255; }

extern "C" size_t sss_jaccard_topk_workspace_bytes(int64_t nq, int64_t n) {
    if (nq <= 0 || n <= 0) return 0;
    return jc_scores_bytes(nq, n) + jc_qsel_bytes(nq) + topk_of_scores_bytes(nq, n);
}

extern "C" int sss_jaccard_topk(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                int64_t n, int k, int64_t id_offset, float* D_out, int64_t* I_out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = jc_sets_ok("jaccard_topk", q_ptr, q_items, nq, c_ptr, c_items, n);
    if (rc) return rc;
    if (k <= 0 || k > JC_MAX_K) { set_error("jaccard_topk: need 0 < k <= 1024"); return SSS_EINVAL; }
    if (!D_out || !I_out || !workspace) {
        set_error("jaccard_topk: a null pointer (D_out, I_out and the workspace are required)");
        return SSS_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("jaccard_topk: workspace must be 256-byte aligned"); return SSS_EINVAL; }
    if (workspace_bytes < sss_jaccard_topk_workspace_bytes(nq, n)) {
        set_error("jaccard_topk: workspace %zu < %zu", workspace_bytes, sss_jaccard_topk_workspace_bytes(nq, n));
        return SSS_EWORKSPACE;
    }
    float* scores = reinterpret_cast<float*>(workspace);
    int* qsel = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + jc_scores_bytes(nq, n));
    void* tail = reinterpret_cast<char*>(qsel) + jc_qsel_bytes(nq);
    int q_per = 0;
    const dim3 grid = jc_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_jaccard_scores, grid, dim3(JC_ROWS), 0, st, q_ptr, q_items, (int)nq, q_per, c_ptr, c_items, n, scores, qsel);
    rc = check_launch("k_jaccard_scores");
    if (rc) return rc;
    return topk_of_scores(scores, qsel, nq, n, k, id_offset, 0, D_out, I_out, tail, st);
}

extern "C" int sss_jaccard_bands(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                 int64_t n, const double* edges, int n_edges, int64_t id_offset, int64_t* counts, int64_t* first,
                                 void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = jc_sets_ok("jaccard_bands", q_ptr, q_items, nq, c_ptr, c_items, n);
    if (rc) return rc;
    if (n_edges < 1 || n_edges > JC_MAX_EDGES) { set_error("jaccard_bands: need 1 <= n_edges <= 7"); return SSS_EINVAL; }
    if (!edges || !counts || !first) {
        set_error("jaccard_bands: a null pointer (edges, counts and first are required)");
        return SSS_EINVAL;
    }
    if (id_offset < 0 || id_offset > INT64_MAX - n) {
        set_error("jaccard_bands: need 0 <= id_offset <= 2^63 - 1 - n (-1 marks a band without a row)");
        return SSS_EINVAL;
    }
    JcEdges E;
    for (int e = 0; e < JC_MAX_EDGES; ++e) {
        E.e[e] = e < n_edges ? edges[e] : (double)INFINITY;
        if (e < n_edges && (!isfinite(E.e[e]) || (e > 0 && !(E.e[e] > E.e[e - 1])))) {
            set_error("jaccard_bands: edges must be finite and strictly ascending (edge %d)", e);
            return SSS_EINVAL;
        }
    }
    const int nb = n_edges + 1;
    const size_t bytes = (size_t)nq * nb * sizeof(int64_t);
    if (hipMemsetAsync(counts, 0, bytes, st) != hipSuccess || hipMemsetAsync(first, 0xFF, bytes, st) != hipSuccess) {
        set_error("jaccard_bands: memset failed");
        return SSS_EHIP;
    }
    int q_per = 0;
    const dim3 grid = jc_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_jaccard_bands, grid, dim3(JC_ROWS), 0, st, q_ptr, q_items, (int)nq, q_per, c_ptr, c_items, n, E, nb, id_offset,
                       reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(first));
    return check_launch("k_jaccard_bands");
}

}  // namespace sss
