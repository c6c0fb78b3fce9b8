// Ground truth over the whole corpus: the item-set Jaccard of a query against every corpus row (the 'all_jaccard' /
// 'cur_jaccard' kinds of the reference's get_score, fine_tune_ours.py:42-55), its exact top-k, and the band counts / first
// rows of the fine-tuning triple mining (fine_tune_ours.py:187-235).  C ABI and THE CONTRACT: include/sss_jaccard.h;
// measurements: DESIGN.md 5.7.
//
// Both kernels are the walk of csr_walk.h over items alone, counting the hits.
//
//   k_jaccard_scores    writes float32(inter / uni) for every pair and the identity query selection; topk_of_scores
//                       (exhaustive.hip, metric 0) is the unchanged tail
//   k_jaccard_bands     no matrix: the band counts of band_count.h (a ballot per band over the wave, an LDS flush, integer
//                       atomics), shared with ptype.hip
#include <math.h>

#include "band_count.h"
#include "scan.h"

namespace sss {

// Items only, no weights: the 32 KiB that hold 16 (item, weight) entries per row in k_sparse_scores hold 32 items here.
// Every row session_vectors builds from the benchmark corpora (at most 19 actions) and all but the longest real sessions
// then take the LDS form; 64 would cover the builder's limit but leaves 2 workgroups a CU (64 KiB each) where 32 leaves 4.
constexpr int JC_D = 32;
constexpr int JC_MAX_K = 1024;        // k_topk_radix's RS_MAX_K

// |Q & C| of the query entries [q0, q1) and the thread's row
template <class View>
__device__ __forceinline__ int jc_inter(const int* __restrict__ qitems, long q0, long q1, const View& V) {
    int acc = 0;
    csr_merge(qitems, q0, q1, V, [&](long, int) { ++acc; });
    return acc;
}

// grid (row blocks, query ranges); block (0, y) also writes the identity query selection the top-k reads.
__global__ __launch_bounds__(CSR_ROWS) void k_jaccard_scores(const long* __restrict__ qptr, const int* __restrict__ qitems, int nq,
                                                             int q_per, const long* __restrict__ cptr, const int* __restrict__ citems,
                                                             long n, float* __restrict__ scores, int* __restrict__ qsel) {
    __shared__ int r_it[JC_D * CSR_ROWS];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * CSR_ROWS + tid;
    CsrRow<JC_D, false> R{citems, nullptr, r_it, nullptr, tid};
    R.stage(cptr, row, n);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    R.each_space([&](auto V) {
        for (int f = f_lo; f < f_hi; ++f) {
            if (blockIdx.x == 0 && tid == 0) qsel[f] = f;
            const long q0 = qptr[f], q1 = q0 + csr_len(q0, qptr[f + 1]);
            const int acc = jc_inter(qitems, q0, q1, V);
            const long uni = (q1 - q0) + R.lr - acc;
            if (row < n) scores[(size_t)f * n + row] = uni ? (float)__ddiv_rn((double)acc, (double)uni) : 0.f;
        }
    });
}

// The band counts of band_count.h (its ballot and its flush) over the score (double)inter / (double)uni.
__global__ __launch_bounds__(CSR_ROWS) void k_jaccard_bands(const long* __restrict__ qptr, const int* __restrict__ qitems, int nq,
                                                            int q_per, const long* __restrict__ cptr, const int* __restrict__ citems,
                                                            long n, const BandEdges E, int nb, long id_offset,
                                                            unsigned long long* __restrict__ counts,
                                                            unsigned long long* __restrict__ first_out) {
    __shared__ int r_it[JC_D * CSR_ROWS];
    __shared__ BandWords s_tot;
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * CSR_ROWS, row = row0 + tid;
    CsrRow<JC_D, false> R{citems, nullptr, r_it, nullptr, tid};
    R.stage(cptr, row, n);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    for (int f0 = f_lo; f0 < f_hi; f0 += BD_QRUN) {              // workgroup-uniform: band_flush's barriers are met by all
        const int fe = f0 + BD_QRUN < f_hi ? f0 + BD_QRUN : f_hi;
        R.each_space([&](auto V) {
            for (int f = f0; f < fe; ++f) {
                const long q0 = qptr[f], q1 = q0 + csr_len(q0, qptr[f + 1]);
                const int acc = jc_inter(qitems, q0, q1, V);
                const long uni = (q1 - q0) + R.lr - acc;
                const double s = uni ? __ddiv_rn((double)acc, (double)uni) : 0.0;
                band_ballot(s_tot, f - f0, row < n, s, E, nb);
            }
        });
        band_flush(s_tot, f0, fe, nb, row0, id_offset, counts, first_out);
    }
}

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

extern "C" size_t sss_jaccard_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

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
    ScoreWs w;
    rc = score_ws_carve("jaccard_topk", workspace, workspace_bytes, nq, n, &w);
    if (rc) return rc;
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_jaccard_scores, grid, dim3(CSR_ROWS), 0, st, q_ptr, q_items, (int)nq, q_per, c_ptr, c_items, n, w.scores, w.qsel);
    return scores_topk("k_jaccard_scores", w, nq, n, k, id_offset, D_out, I_out, st);
}

extern "C" int sss_jaccard_bands(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                 int64_t n, const double* edges, int n_edges, int64_t id_offset, int64_t* counts, int64_t* first,
                                 void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = jc_sets_ok("jaccard_bands", q_ptr, q_items, nq, c_ptr, c_items, n);
    if (rc) return rc;
    BandEdges E;
    rc = band_args("jaccard_bands", edges, n_edges, id_offset, nq, n, counts, first, &E, st);
    if (rc) return rc;
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_jaccard_bands, grid, dim3(CSR_ROWS), 0, st, q_ptr, q_items, (int)nq, q_per, c_ptr, c_items, n, E, n_edges + 1, id_offset,
                       reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(first));
    return check_launch("k_jaccard_bands");
}

}  // namespace sss
