// Ground truth over the whole corpus: the item-set Jaccard of a query against every corpus row (the 'all_jaccard' /
// 'cur_jaccard' kinds of the reference's get_score, fine_tune_ours.py:42-55), its exact top-k, and the band counts / first
// rows of the fine-tuning triple mining (fine_tune_ours.py:187-235).  C ABI and THE CONTRACT: include/sss_jaccard.h;
// measurements: DESIGN.md 5.7.
//
// Both kernels are a frame under JaccardKind, the walk of csr_walk.h over items alone, counting the hits.
//
//   k_jaccard_scores    csr_walk.h's score frame: float32(inter / uni) for every pair and the identity query selection;
//                       topk_of_scores (topk_scores.hip, metric 0) is the unchanged tail
//   k_jaccard_bands     band_count.h's band frame: no matrix, a ballot per band over the wave, an LDS flush, integer atomics
//
// The host piece band_count.h declares for the two *_bands entry points (this one and ptype.hip's) is below.
#include <math.h>

#include "band_count.h"

namespace sss {

// |Q & C| of the query entries [q0, q1) and the thread's row
template <class View>
__device__ __forceinline__ int jc_inter(const int* __restrict__ qitems, long q0, long q1, const View& V) {
    int acc = 0;
    csr_merge(qitems, q0, q1, V, [&](long, int) { ++acc; });
    return acc;
}

// score = (double)inter / (double)uni, 0 for an empty union (then inter is 0 too, and 0 / 1 is that 0: the division is the
// whole wave's, with no branch around it).  Items only, no weights: the 32 KiB that hold 16 (item, weight)
// entries per row in k_sparse_scores hold 32 items here.  Every row session_vectors builds from the benchmark corpora (at
// most 19 actions) and all but the longest real sessions then take the LDS form; 64 would cover the builder's limit but
// leaves 2 workgroups a CU (64 KiB each) where 32 leaves 4.
constexpr int JC_D = 32;

struct JaccardKind {
    static constexpr int DEPTH = JC_D;
    static constexpr bool WEIGHTS = false;
    __device__ static NoRowState row_state(const CsrRow<DEPTH, WEIGHTS>&) { return {}; }
    template <class View>
    __device__ static double pair(const CsrSets& Q, long q0, int ql, const View& V, NoRowState) {
        const int acc = jc_inter(Q.items, q0, q0 + ql, V);
        const long uni = (long)ql + V.lr - acc;
        return __ddiv_rn((double)acc, (double)(uni ? uni : 1));
    }
};

// Both take the weight pointers every kind's kernel takes (csr_walk.h's ScoreKernel, band_count.h's BandKernel) and read neither.
__global__ __launch_bounds__(CSR_ROWS) void k_jaccard_scores(const long* __restrict__ qptr, const int* __restrict__ qitems, const float*,
                                                             int nq, int q_per, const long* __restrict__ cptr,
                                                             const int* __restrict__ citems, const float*, long n,
                                                             float* __restrict__ scores, int* __restrict__ qsel) {
    csr_scores<JaccardKind>({qptr, qitems, nullptr}, nq, q_per, {cptr, citems, nullptr}, n, scores, qsel);
}

__global__ __launch_bounds__(CSR_ROWS) void k_jaccard_bands(const long* __restrict__ qptr, const int* __restrict__ qitems, const float*,
                                                            int nq, int q_per, const long* __restrict__ cptr,
                                                            const int* __restrict__ citems, const float*, long n,
                                                            const BandEdges E, int nb, long id_offset,
                                                            unsigned long long* __restrict__ counts,
                                                            unsigned long long* __restrict__ first_out) {
    csr_bands<JaccardKind>({qptr, qitems, nullptr}, nq, q_per, {cptr, citems, nullptr}, n, E, nb, id_offset, counts, first_out);
}

// ------------------------------------------------------------------------------ host launchers
// ---- the host piece declared in band_count.h (ptype.hip's entry point uses it too)
int band_counts(const char* what, const char* name, BandKernel kernel, const CsrSets& Q, long nq, const CsrSets& C, long n, bool weighted,
                const double* edges, int n_edges, long id_offset, int64_t* counts, int64_t* first, hipStream_t st) {
    const int rc = csr_args_ok(what, Q, nq, 65535, C, n, weighted);
    if (rc) return rc;
    if (n_edges < 1 || n_edges > BD_MAX_EDGES) { set_error("%s: need 1 <= n_edges <= 7", what); return SSS_EINVAL; }
    if (!edges || !counts || !first) {
        set_error("%s: a null pointer (edges, counts and first are required)", what);
        return SSS_EINVAL;
    }
    if (id_offset < 0 || id_offset > INT64_MAX - n) {
        set_error("%s: need 0 <= id_offset <= 2^63 - 1 - n (-1 marks a band without a row)", what);
        return SSS_EINVAL;
    }
    BandEdges E;
    for (int e = 0; e < BD_MAX_EDGES; ++e) {
        E.e[e] = e < n_edges ? edges[e] : (double)INFINITY;
        if (e < n_edges && (!isfinite(E.e[e]) || (e > 0 && !(E.e[e] > E.e[e - 1])))) {
            set_error("%s: edges must be finite and strictly ascending (edge %d)", what, e);
            return SSS_EINVAL;
        }
    }
    const size_t bytes = (size_t)nq * (n_edges + 1) * sizeof(int64_t);
    if (hipMemsetAsync(counts, 0, bytes, st) != hipSuccess || hipMemsetAsync(first, 0xFF, bytes, st) != hipSuccess) {
        set_error("%s: memset failed", what);
        return SSS_EHIP;
    }
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(kernel, grid, dim3(CSR_ROWS), 0, st, Q.ptr, Q.items, Q.w, (int)nq, q_per, C.ptr, C.items, C.w, n, E, n_edges + 1,
                       id_offset, reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(first));
    return check_launch(name);
}

extern "C" size_t sss_jaccard_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

extern "C" int sss_jaccard_topk(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                int64_t n, int k, int64_t id_offset, float* D_out, int64_t* I_out, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return score_topk("jaccard_topk", "k_jaccard_scores", k_jaccard_scores, {q_ptr, q_items, nullptr}, nq, {c_ptr, c_items, nullptr}, n, false, k,
                      id_offset, D_out, I_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int sss_jaccard_bands(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                 int64_t n, const double* edges, int n_edges, int64_t id_offset, int64_t* counts, int64_t* first,
                                 void* stream) {
    return band_counts("jaccard_bands", "k_jaccard_bands", k_jaccard_bands, {q_ptr, q_items, nullptr}, nq, {c_ptr, c_items, nullptr}, n, false, edges,
                       n_edges, id_offset, counts, first, static_cast<hipStream_t>(stream));
}

}  // namespace sss
