// Sparse session vectors over the item vocabulary and their exact top-k: the reference's SKNN / STAN item-vector
// baselines (test_amazon_filterd.py: sequence_to_binary_vec :48-57, sequence_to_stan_vec :37-46,
// find_K_sparse_dense :403-412, the 'SKNN' / 'STAN' branch of main2 :582-603).  C ABI: include/sss_sparse.h.
//
// A session vector is a CSR row: the session's distinct item ids ascending (int32) with one float32 weight each,
// computed in float64 and rounded once (DESIGN.md "sparse session index").  The canonical score of (query, row) is the
// float64 sum of (double)wq * (double)wc over the shared items in ascending item order, rounded once to float32; the
// result is the k best rows by (score desc, id asc).  No floating-point atomics anywhere: every score is one thread's
// sequential sum, so results are bit-reproducible.
//
//   k_svec_count / k_svec_fill         one wave per session: session_lane.h's compaction and ranks over item ids, float64
//                                      weights
//   k_sparse_scores                    csr_walk.h's score frame under SparseKind: one thread per corpus row, stores
//                                      coalesced across rows
//   topk_of_scores (topk_scores.hip)   the exact top-k of the score matrix, shared with the dense exhaustive search
//
// The host pieces csr_walk.h declares for the three *_topk entry points (this one, jaccard.hip's, ptype.hip's) are below.
#include <math.h>

#include "csr_walk.h"
#include "scan.h"
#include "session_lane.h"

namespace sss {

constexpr int SP_MAX_K = 1024;        // k_topk_radix's RS_MAX_K

struct InvSqrtTable { float v[SL_MAX_ITEMS + 1]; };   // v[m] = float(1 / sqrt(double(m))), made on the host

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// The wave's session with item ids on the lanes (err bit 1: an item id outside [0, n_items)), ranked; *u (stan): the sum
// over the item's occurrences of exp((i - L) / lammy), added in action order.
__device__ __forceinline__ SessionLane item_lane(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                 const long* __restrict__ item_id, long s, long n_items, int stan, double lammy,
                                                 int* __restrict__ err, double* u) {
    SessionLane Ln = session_compact(sess_ptr, is_search, item_id, s, err, [&](long it, int& bad) {
        if (it < 0 || it >= n_items) bad |= 2;
        return (int)it;
    });
    *u = 0.0;
    const double w = (Ln.t < Ln.L && stan) ? exp((double)(Ln.t - Ln.L) / lammy) : 0.0;
    session_rank(Ln, [&](int a, bool hit) {
        const double wa = stan ? readlane_f64(w, a) : 0.0;
        if (hit) *u += wa;
    });
    return Ln;
}

__global__ __launch_bounds__(256) void k_svec_count(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                    const long* __restrict__ item_id, long S, long n_items,
                                                    int* __restrict__ counts, int* __restrict__ err) {
    const long s = session_of_wave();
    if (s >= S) return;
    double u;
    const SessionLane Ln = item_lane(sess_ptr, is_search, item_id, s, n_items, 0, 1.0, err, &u);
    if (Ln.t == 0) counts[s] = Ln.m;
}

__global__ __launch_bounds__(256) void k_svec_fill(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                   const long* __restrict__ item_id, long S, long n_items, int stan, double lammy,
                                                   const InvSqrtTable tab, const long* __restrict__ ptr, int* __restrict__ items,
                                                   float* __restrict__ weights, int* __restrict__ err) {
    const long s = session_of_wave();
    if (s >= S) return;
    double u;
    const SessionLane Ln = item_lane(sess_ptr, is_search, item_id, s, n_items, stan, lammy, err, &u);
    float w = tab.v[Ln.m];
    if (stan) {
        double ss = 0.0;                                         // sum of u^2 in ascending item order
        for (int r = 0; r < Ln.m; ++r) {
            const unsigned long long who = __builtin_amdgcn_ballot_w64(Ln.first && Ln.rank == r);
            const double ur = readlane_f64(u, __builtin_ctzll(who));
            ss += ur * ur;
        }
        w = (float)__ddiv_rn(u, __dsqrt_rn(ss));
    }
    if (Ln.first) {
        const long at = ptr[s] + Ln.rank;
        items[at] = Ln.value;
        weights[at] = w;
    }
}

// ---- score = the float64 sum over the shared items, ascending, of (double)wq * (double)wc; SP_RL (item, weight) entries of
// a row staged.
constexpr int SP_RL = 16;

struct SparseKind {
    static constexpr int DEPTH = SP_RL;
    static constexpr bool WEIGHTS = true;
    __device__ static NoRowState row_state(const CsrRow<DEPTH, WEIGHTS>&) { return {}; }
    template <class View>
    __device__ static double pair(const CsrSets& Q, long q0, int ql, const View& V, NoRowState) {
        double acc = 0.0;
        csr_merge(Q.items, q0, q0 + ql, V, [&](long p, int j) { acc += (double)Q.w[p] * (double)V.weight(j); });
        return acc;
    }
};

__global__ __launch_bounds__(CSR_ROWS) void k_sparse_scores(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                            const float* __restrict__ qw, int nq, int q_per,
                                                            const long* __restrict__ cptr, const int* __restrict__ citems,
                                                            const float* __restrict__ cw, long n, float* __restrict__ scores,
                                                            int* __restrict__ qsel) {
    csr_scores<SparseKind>({qptr, qitems, qw}, nq, q_per, {cptr, citems, cw}, n, scores, qsel);
}

// ------------------------------------------------------------------------------ host launchers
extern "C" int sss_session_vectors_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                         int64_t n_items, int32_t* counts, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned nb = 0;
    int rc = session_args("session_vectors_count", sess_ptr, is_search, item_id, n_sessions, n_items, err, &nb);
    if (rc) return rc;
    if (!counts) { set_error("session_vectors_count: a null pointer (counts is required)"); return SSS_EINVAL; }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("session_vectors_count: memset failed"); return SSS_EHIP; }
    hipLaunchKernelGGL(k_svec_count, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, n_items, counts, err);
    return check_launch("k_svec_count");
}

extern "C" int sss_session_vectors_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                        int64_t n_items, int mode, double lammy, const int64_t* ptr, int32_t* items, float* weights,
                                        int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned nb = 0;
    int rc = session_args("session_vectors_fill", sess_ptr, is_search, item_id, n_sessions, n_items, err, &nb);
    if (rc) return rc;
    if ((mode != 0 && mode != 1) || (mode == 1 && !(lammy > 0.0 && lammy <= 1.7976931348623157e308))) {
        set_error("session_vectors_fill: mode is 0 (binary) or 1 (stan, with a finite lammy > 0)");
        return SSS_EINVAL;
    }
    if (!ptr || !items || !weights) { set_error("session_vectors_fill: a null pointer (ptr, items and weights are required)"); return SSS_EINVAL; }
    InvSqrtTable tab;
    tab.v[0] = 0.f;
    for (int m = 1; m <= SL_MAX_ITEMS; ++m) tab.v[m] = (float)(1.0 / sqrt((double)m));
    hipLaunchKernelGGL(k_svec_fill, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, n_items, mode, lammy, tab, ptr, items,
                       weights, err);
    return check_launch("k_svec_fill");
}

// ---- the host pieces declared in csr_walk.h (jaccard.hip's and ptype.hip's entry points use them too)
int csr_args_ok(const char* what, const CsrSets& Q, long nq, long nq_max, const CsrSets& C, long n, bool weighted) {
    if (nq <= 0 || nq > nq_max || n <= 0 || n >= (1L << 31)) {
        if (nq_max == 65535) set_error("%s: need 0 < nq <= 65535, 0 < n < 2^31", what);
        else set_error("%s: need 0 < nq < 2^31, 0 < n < 2^31", what);
        return SSS_EINVAL;
    }
    if (!Q.ptr || !Q.items || !C.ptr || !C.items || (weighted && (!Q.w || !C.w))) {
        set_error("%s: a null pointer (ptr and items%s of both the queries and the corpus are required)", what, weighted ? ", weights" : "");
        return SSS_EINVAL;
    }
    return SSS_OK;
}

dim3 csr_grid(long nq, long n, int* q_per) {
    const long nbx = (n + CSR_ROWS - 1) / CSR_ROWS;
    long ny = (1024 + nbx - 1) / nbx;
    if (ny > nq) ny = nq;
    *q_per = (int)((nq + ny - 1) / ny);
    ny = (nq + *q_per - 1) / *q_per;
    return dim3((unsigned)nbx, (unsigned)ny);
}

static size_t ws_qsel_bytes(long nq) { return al256((size_t)nq * 4); }

size_t score_ws_bytes(long nq, long n) {
    if (nq <= 0 || n <= 0) return 0;
    return score_matrix_bytes(nq, n) + ws_qsel_bytes(nq) + topk_of_scores_bytes(nq, n);
}

int score_topk(const char* what, const char* name, ScoreKernel kernel, const CsrSets& Q, long nq, const CsrSets& C, long n,
               bool weighted, int k, long id_offset, float* D_out, long* I_out, void* workspace, size_t workspace_bytes, hipStream_t st) {
    int rc = csr_args_ok(what, Q, nq, 65535, C, n, weighted);
    if (rc) return rc;
    if (k <= 0 || k > SP_MAX_K) { set_error("%s: need 0 < k <= 1024", what); return SSS_EINVAL; }
    if (!D_out || !I_out || !workspace) {
        set_error("%s: a null pointer (D_out, I_out and the workspace are required)", what);
        return SSS_EINVAL;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("%s: workspace must be 256-byte aligned", what); return SSS_EINVAL; }
    if (workspace_bytes < score_ws_bytes(nq, n)) {
        set_error("%s: workspace %zu < %zu", what, workspace_bytes, score_ws_bytes(nq, n));
        return SSS_EWORKSPACE;
    }
    float* scores = reinterpret_cast<float*>(workspace);
    int* qsel = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + score_matrix_bytes(nq, n));
    void* tail = reinterpret_cast<char*>(qsel) + ws_qsel_bytes(nq);
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(kernel, grid, dim3(CSR_ROWS), 0, st, Q.ptr, Q.items, Q.w, (int)nq, q_per, C.ptr, C.items, C.w, n, scores, qsel);
    rc = check_launch(name);
    if (rc) return rc;
    return topk_of_scores(scores, qsel, nq, n, k, id_offset, 0, D_out, I_out, tail, st);
}

extern "C" size_t sss_sparse_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

extern "C" int sss_sparse_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                               const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                               int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream) {
    return score_topk("sparse_topk", "k_sparse_scores", k_sparse_scores, {q_ptr, q_items, q_weights}, nq, {c_ptr, c_items, c_weights}, n, true, k,
                      id_offset, D_out, I_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

}  // namespace sss
