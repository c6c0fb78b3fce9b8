// Ground truth under the product-type kind, the similarity the reference is configured with (config.py:61,
// 'all_product_type_score' of get_score, fine_tune_ours.py:66-85): the cosine of two sessions' product-type count vectors
// over the whole corpus -- the bags, their exact top-k, the band counts / first rows of the triple mining, and the pair
// scores of a result.  C ABI and THE CONTRACT: include/sss_ptype.h; measurements: DESIGN.md 5.11.
//
// A type bag is a CSR row of (type id ascending, count as an exact float32).  Every score is integer arithmetic
// (dot, nq2, nc2), one correctly rounded square root and one correctly rounded division.
//
//   k_tbag_count / k_tbag_fill   one wave per session: session_lane.h's compaction and ranks over the actions' types
//                                (through item_type), the multiplicity counted over equal types
//   k_ptype_scores               csr_walk.h's score frame under PtypeKind, the walk over (type, count) entries: a thread
//                                owns a corpus row and takes its nc2 once after staging; the query's nq2 is wave-uniform;
//                                float32(score) and the identity query selection; topk_of_scores (topk_scores.hip, metric 0)
//                                is the unchanged tail
//   k_ptype_bands                band_count.h's band frame under PtypeKind: no matrix, the float64 score itself
//   k_ptype_pair_scores          one wave per query, lane l owns the neighbours j = l, l + 64, ... (as k_item_overlap): one
//                                short sorted merge per pair, the float64 score itself
#include <math.h>

#include "band_count.h"
#include "session_lane.h"

namespace sss {

constexpr int PT_D = 16;              // (type, count) entries of a row staged in LDS: SparseKind's SP_RL
constexpr int PT_MAX_K = 1024;       // k_topk_radix's RS_MAX_K
constexpr int PT_WAVES = 4;           // queries per workgroup of k_ptype_pair_scores

// The wave's session with types on the lanes (err bit 1: an item id outside [0, n_items); bit 2: a type id outside
// [-1, n_types); an untyped item counts for nothing), ranked; *count: the session's item actions of the lane's type.
__device__ __forceinline__ SessionLane type_lane(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                 const long* __restrict__ item_id, long s, const int* __restrict__ item_type,
                                                 long n_items, long n_types, int* __restrict__ err, int* count) {
    SessionLane Ln = session_compact(sess_ptr, is_search, item_id, s, err, [&](long it, int& bad) {
        if (it < 0 || it >= n_items) {
            bad |= 2;
            return -1;
        }
        const int ty = item_type[it];
        if (ty < -1 || ty >= n_types) {
            bad |= 4;
            return -1;
        }
        return ty;
    });
    *count = 0;
    session_rank(Ln, [&](int, bool hit) {
        if (hit) ++*count;
    });
    return Ln;
}

__global__ __launch_bounds__(256) void k_tbag_count(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                    const long* __restrict__ item_id, long S, const int* __restrict__ item_type,
                                                    long n_items, long n_types, int* __restrict__ counts, int* __restrict__ err) {
    const long s = session_of_wave();
    if (s >= S) return;
    int count;
    const SessionLane Ln = type_lane(sess_ptr, is_search, item_id, s, item_type, n_items, n_types, err, &count);
    if (Ln.t == 0) counts[s] = Ln.m;
}

__global__ __launch_bounds__(256) void k_tbag_fill(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                   const long* __restrict__ item_id, long S, const int* __restrict__ item_type,
                                                   long n_items, long n_types, const long* __restrict__ ptr, int* __restrict__ items,
                                                   float* __restrict__ weights, int* __restrict__ err) {
    const long s = session_of_wave();
    if (s >= S) return;
    int count;
    const SessionLane Ln = type_lane(sess_ptr, is_search, item_id, s, item_type, n_items, n_types, err, &count);
    if (Ln.first) {
        const long at = ptr[s] + Ln.rank;
        items[at] = Ln.value;
        weights[at] = (float)count;
    }
}

// ---- the score of record.  Counts are exact integers in float32; a valid bag's sum of squares is <= 2^26, so dot < 2^31 and
// nq2 * nc2 <= 2^52 is exact in a double.
__device__ __forceinline__ long pt_sq(float w) {
    const int c = (int)w;
    return (long)c * c;
}

__device__ __forceinline__ double pt_score(long dot, long nq2, long nc2) {
    return dot == 0 ? 0.0 : __ddiv_rn((double)dot, __dsqrt_rn((double)(nq2 * nc2)));
}

// sum of squared counts of the query entries [q0, q1): the same for the whole wave (uniform loads)
__device__ __forceinline__ long pt_norm2(const float* __restrict__ qw, long q0, long q1) {
    long s = 0;
    for (long p = q0; p < q1; ++p) s += pt_sq(qw[p]);
    return s;
}

// score = pt_score of the pair's dot and the two sums of squares; the row state is the row's nc2.
struct PtypeKind {
    static constexpr int DEPTH = PT_D;
    static constexpr bool WEIGHTS = true;
    // the staged entries from the thread's LDS column, the rest of a row longer than the column from global memory
    __device__ static long row_state(const CsrRow<DEPTH, WEIGHTS>& R) {
        long s = 0;
        for (int j = 0; j < DEPTH && j < R.lr; ++j) s += pt_sq(R.s_w[j * CSR_ROWS + R.tid]);
        for (int j = DEPTH; j < R.lr; ++j) s += pt_sq(R.cw[R.r0 + j]);
        return s;
    }
    template <class View>
    __device__ static double pair(const CsrSets& Q, long q0, int ql, const View& V, long nc2) {
        const long q1 = q0 + ql;
        long dot = 0;
        csr_merge(Q.items, q0, q1, V, [&](long p, int j) { dot += (long)(int)Q.w[p] * (int)V.weight(j); });
        return pt_score(dot, pt_norm2(Q.w, q0, q1), nc2);
    }
};

__global__ __launch_bounds__(CSR_ROWS) void k_ptype_scores(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                           const float* __restrict__ qw, int nq, int q_per,
                                                           const long* __restrict__ cptr, const int* __restrict__ citems,
                                                           const float* __restrict__ cw, long n, float* __restrict__ scores,
                                                           int* __restrict__ qsel) {
    csr_scores<PtypeKind>({qptr, qitems, qw}, nq, q_per, {cptr, citems, cw}, n, scores, qsel);
}

__global__ __launch_bounds__(CSR_ROWS) void k_ptype_bands(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                          const float* __restrict__ qw, int nq, int q_per,
                                                          const long* __restrict__ cptr, const int* __restrict__ citems,
                                                          const float* __restrict__ cw, long n, const BandEdges E, int nb,
                                                          long id_offset, unsigned long long* __restrict__ counts,
                                                          unsigned long long* __restrict__ first_out) {
    csr_bands<PtypeKind>({qptr, qitems, qw}, nq, q_per, {cptr, citems, cw}, n, E, nb, id_offset, counts, first_out);
}

// One wave per query; lane l owns the neighbours j = l, l + 64, ...  The query's entries are the same for the whole wave
// (uniform loads); each lane advances through its neighbour's row in global memory as the query's types ascend.  Every
// (i, j) has one owner; the only atomic is the OR into err.
__global__ __launch_bounds__(PT_WAVES * 64) void k_ptype_pair_scores(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                                    const float* __restrict__ qw, long nq,
                                                                    const long* __restrict__ cptr, const int* __restrict__ citems,
                                                                    const float* __restrict__ cw, long n, const long* __restrict__ I,
                                                                    int K, long id_offset, double* __restrict__ scores,
                                                                    int* __restrict__ err) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * PT_WAVES + (threadIdx.x >> 6);
    if (i >= nq) return;                                             // whole wave; no barrier below
    const long q0 = qptr[i], q1 = q0 + csr_len(q0, qptr[i + 1]);
    const long nq2 = pt_norm2(qw, q0, q1);
    bool bad = false;
    for (int jb = 0; jb < K; jb += 64) {                             // wave-uniform trip count
        const int j = jb + lane;
        long c0 = 0;
        int len = -1;
        if (j < K) len = csr_neighbour(cptr, n, I[(size_t)i * K + j], id_offset, &c0, &bad);
        const int lr = len < 0 ? 0 : len;                            // a missing neighbour walks nothing
        long nc2 = 0, dot = 0;
        for (int e = 0; e < lr; ++e) nc2 += pt_sq(cw[c0 + e]);
        auto item_at = [&](int e) { return citems[c0 + e]; };
        auto weight_at = [&](int e) { return cw[c0 + e]; };
        const CsrView<decltype(item_at), decltype(weight_at)> V{lr, lr > 0 ? item_at(0) : CSR_END, item_at, weight_at};
        csr_merge(qitems, q0, q1, V, [&](long p, int e) { dot += (long)(int)qw[p] * (int)V.weight(e); });
        if (j < K) scores[(size_t)i * K + j] = len < 0 ? (double)NAN : pt_score(dot, nq2, nc2);
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicOr(err, 1);
}

// ------------------------------------------------------------------------------ host launchers
// session_lane.h's builder arguments and the type table's; *nb: the workgroups of the launch
static int tbag_args(const char* what, const void* sess_ptr, const void* is_search, const void* item_id, long S, const void* item_type,
                     long n_items, long n_types, const void* err, unsigned* nb) {
    const int rc = session_args(what, sess_ptr, is_search, item_id, S, n_items, err, nb);
    if (rc) return rc;
    if (n_types <= 0 || n_types > 0x7fffffffL) { set_error("%s: need 0 < n_types < 2^31", what); return SSS_EINVAL; }
    if (!item_type) { set_error("%s: a null pointer (item_type is required)", what); return SSS_EINVAL; }
    return SSS_OK;
}

extern "C" int sss_type_bags_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                   const int32_t* item_type, int64_t n_items, int64_t n_types, int32_t* counts, int32_t* err,
                                   void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned nb = 0;
    int rc = tbag_args("type_bags_count", sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, err, &nb);
    if (rc) return rc;
    if (!counts) { set_error("type_bags_count: a null pointer (counts is required)"); return SSS_EINVAL; }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("type_bags_count: memset failed"); return SSS_EHIP; }
    hipLaunchKernelGGL(k_tbag_count, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, counts,
                       err);
    return check_launch("k_tbag_count");
}

extern "C" int sss_type_bags_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                  const int32_t* item_type, int64_t n_items, int64_t n_types, const int64_t* ptr, int32_t* items,
                                  float* weights, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    unsigned nb = 0;
    int rc = tbag_args("type_bags_fill", sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, err, &nb);
    if (rc) return rc;
    if (!ptr || !items || !weights) { set_error("type_bags_fill: a null pointer (ptr, items and weights are required)"); return SSS_EINVAL; }
    hipLaunchKernelGGL(k_tbag_fill, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, ptr,
                       items, weights, err);
    return check_launch("k_tbag_fill");
}

extern "C" size_t sss_ptype_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

extern "C" int sss_ptype_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                              const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                              int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream) {
    return score_topk("ptype_topk", "k_ptype_scores", k_ptype_scores, {q_ptr, q_items, q_weights}, nq, {c_ptr, c_items, c_weights}, n, true, k,
                      id_offset, D_out, I_out, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

extern "C" int sss_ptype_bands(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                               const int32_t* c_items, const float* c_weights, int64_t n, const double* edges, int n_edges,
                               int64_t id_offset, int64_t* counts, int64_t* first, void* stream) {
    return band_counts("ptype_bands", "k_ptype_bands", k_ptype_bands, {q_ptr, q_items, q_weights}, nq, {c_ptr, c_items, c_weights}, n, true, edges,
                       n_edges, id_offset, counts, first, static_cast<hipStream_t>(stream));
}

extern "C" int sss_ptype_pair_scores(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                                     const int32_t* c_items, const float* c_weights, int64_t n, const int64_t* I, int K, int64_t id_offset,
                                     double* scores, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = csr_args_ok("ptype_pair_scores", {q_ptr, q_items, q_weights}, nq, (1L << 31) - 1, {c_ptr, c_items, c_weights}, n, true);
    if (rc) return rc;
    if (K <= 0 || K > PT_MAX_K) { set_error("ptype_pair_scores: need 0 < K <= 1024"); return SSS_EINVAL; }
    if (!I || !scores || !err) { set_error("ptype_pair_scores: a null pointer (I, scores and err are required)"); return SSS_EINVAL; }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("ptype_pair_scores: memset failed"); return SSS_EHIP; }
    const unsigned nb = (unsigned)((nq + PT_WAVES - 1) / PT_WAVES);
    hipLaunchKernelGGL(k_ptype_pair_scores, dim3(nb), dim3(PT_WAVES * 64), 0, st, q_ptr, q_items, q_weights, nq, c_ptr, c_items, c_weights, n,
                       I, K, id_offset, scores, err);
    return check_launch("k_ptype_pair_scores");
}

}  // namespace sss
