// Ground truth under the product-type kind, the similarity the reference is configured with (config.py:61,
// 'all_product_type_score' of get_score, fine_tune_ours.py:66-85): the cosine of two sessions' product-type count vectors
// over the whole corpus -- the bags, their exact top-k, the band counts / first rows of the triple mining, and the pair
// scores of a result.  C ABI and THE CONTRACT: include/sss_ptype.h; measurements: DESIGN.md 5.11.
//
// A type bag is a CSR row of (type id ascending, count as an exact float32).  Every score is integer arithmetic
// (dot, nq2, nc2), one correctly rounded square root and one correctly rounded division.
//
//   k_tbag_count / k_tbag_fill   one wave per session, one lane per item action (as k_svec_*): the action's type through
//                                item_type, "seen before", multiplicity and rank by readlane broadcasts
//   k_ptype_scores               the walk of csr_walk.h over (type, count) entries: a thread owns a corpus row and takes its
//                                nc2 once after staging; the query's nq2 is wave-uniform; writes float32(score) and the
//                                identity query selection; topk_of_scores (exhaustive.hip, metric 0) is the unchanged tail
//   k_ptype_bands                no matrix: the ballot and the flush of band_count.h over the float64 score
//   k_ptype_pair_scores          one wave per query, lane l owns the neighbours j = l, l + 64, ... (as k_item_overlap): one
//                                short sorted merge per pair, the float64 score itself
#include <math.h>

#include "band_count.h"
#include "scan.h"

namespace sss {

constexpr int TB_MAX_ITEMS = 64;      // item actions per session (one lane each), sss_session_vectors_*'s limit
constexpr int PT_D = 16;              // (type, count) entries of a row staged in LDS: k_sparse_scores' SP_RL
constexpr int PT_MAX_K = 1024;        // k_topk_radix's RS_MAX_K
constexpr int PT_WAVES = 4;           // queries per workgroup of k_ptype_pair_scores

struct TypeLane {
    int m;             // distinct types of the session (0 for a flagged session)
    bool first;        // this lane holds the first occurrence of its type
    int type, rank;    // ... that type and its position in ascending type order
    int count;         // ... and the session's item actions of that type
};

// Lane t of the wave <- the t-th item action of session s (searches skipped; `slot`: 64 ints of LDS owned by the wave),
// as its type.  err bit 0: more than 64 item actions (or a decreasing sess_ptr); bit 1: an item id outside [0, n_items);
// bit 2: a type id outside [-1, n_types).  A flagged session counts as empty, in the count and in the fill alike, so every
// write stays inside the session's own range.
__device__ __forceinline__ TypeLane type_lane(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                              const long* __restrict__ item_id, long s, int t, const int* __restrict__ item_type,
                                              long n_items, long n_types, volatile int* slot, int* __restrict__ err) {
    TypeLane S;
    const long a0 = sess_ptr[s], a1 = sess_ptr[s + 1];
    const unsigned long long lt = t == 0 ? 0ull : (~0ull >> (64 - t));
    int L = 0;
    bool bad_item = false, bad_type = false;
    for (long base = a0; base < a1; base += 64) {                // wave-uniform trip count
        const long a = base + t;
        const bool clk = a < a1 && is_search[a] == 0;
        const long it = clk ? item_id[a] : 0;
        const unsigned long long cm = __builtin_amdgcn_ballot_w64(clk);
        const int dest = L + __builtin_popcountll(cm & lt);
        if (clk) {
            int ty = -1;
            if (it < 0 || it >= n_items) {
                bad_item = true;
            } else {
                ty = item_type[it];
                if (ty < -1 || ty >= n_types) {
                    bad_type = true;
                    ty = -1;
                }
            }
            if (dest < TB_MAX_ITEMS) slot[dest] = ty;
        }
        L += __builtin_popcountll(cm);
    }
    __builtin_amdgcn_wave_barrier();
    int flags = (L > TB_MAX_ITEMS || a1 < a0) ? 1 : 0;
    if (__builtin_amdgcn_ballot_w64(bad_item) != 0ull) flags |= 2;
    if (__builtin_amdgcn_ballot_w64(bad_type) != 0ull) flags |= 4;
    if (flags) {
        if (t == 0) atomicOr(err, flags);
        L = 0;
    }
    S.type = t < L ? slot[t] : -1;
    __builtin_amdgcn_wave_barrier();
    const bool typed = S.type >= 0;
    bool seen = false;
    S.count = 0;
    for (int u = 0; u < L; ++u) {                                // uniform loop: broadcast item action u
        const int tu = __builtin_amdgcn_readlane(S.type, u);
        if (typed && tu == S.type) {
            if (u < t) seen = true;
            ++S.count;
        }
    }
    S.first = typed && !seen;
    const unsigned long long fm = __builtin_amdgcn_ballot_w64(S.first);
    S.m = __builtin_popcountll(fm);
    S.rank = 0;
    for (unsigned long long todo = fm; todo; todo &= todo - 1) {
        const int tu = __builtin_amdgcn_readlane(S.type, __builtin_ctzll(todo));
        if (S.first && tu < S.type) ++S.rank;
    }
    return S;
}

__global__ __launch_bounds__(256) void k_tbag_count(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                    const long* __restrict__ item_id, long S, const int* __restrict__ item_type,
                                                    long n_items, long n_types, int* __restrict__ counts, int* __restrict__ err) {
    __shared__ int slots[4 * TB_MAX_ITEMS];
    const long s = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int t = threadIdx.x & 63;
    if (s >= S) return;                                          // whole wave
    const TypeLane Ln = type_lane(sess_ptr, is_search, item_id, s, t, item_type, n_items, n_types, slots + (threadIdx.x >> 6) * TB_MAX_ITEMS, err);
    if (t == 0) counts[s] = Ln.m;
}

__global__ __launch_bounds__(256) void k_tbag_fill(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                   const long* __restrict__ item_id, long S, const int* __restrict__ item_type,
                                                   long n_items, long n_types, const long* __restrict__ ptr, int* __restrict__ items,
                                                   float* __restrict__ weights, int* __restrict__ err) {
    __shared__ int slots[4 * TB_MAX_ITEMS];
    const long s = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int t = threadIdx.x & 63;
    if (s >= S) return;
    const TypeLane Ln = type_lane(sess_ptr, is_search, item_id, s, t, item_type, n_items, n_types, slots + (threadIdx.x >> 6) * TB_MAX_ITEMS, err);
    if (Ln.first) {
        const long at = ptr[s] + Ln.rank;
        items[at] = Ln.type;
        weights[at] = (float)Ln.count;
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

// The thread's staged row: its nc2, taken once -- the staged entries from the thread's LDS column, the rest of a row longer
// than the column from global memory.
__device__ __forceinline__ long pt_row_norm2(const CsrRow<PT_D, true>& R) {
    long s = 0;
    for (int j = 0; j < PT_D && j < R.lr; ++j) s += pt_sq(R.s_w[j * CSR_ROWS + R.tid]);
    for (int j = PT_D; j < R.lr; ++j) s += pt_sq(R.cw[R.r0 + j]);
    return s;
}

// score of (query f, the thread's row) on one view of the row
template <class View>
__device__ __forceinline__ double pt_pair(const long* __restrict__ qptr, const int* __restrict__ qitems, const float* __restrict__ qw,
                                          int f, const View& V, long nc2) {
    const long q0 = qptr[f], q1 = q0 + csr_len(q0, qptr[f + 1]);
    long dot = 0;
    csr_merge(qitems, q0, q1, V, [&](long p, int j) { dot += (long)(int)qw[p] * (int)V.weight(j); });
    return pt_score(dot, pt_norm2(qw, q0, q1), nc2);
}

// grid (row blocks, query ranges); block (0, y) also writes the identity query selection the top-k reads.
__global__ __launch_bounds__(CSR_ROWS) void k_ptype_scores(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                           const float* __restrict__ qw, int nq, int q_per,
                                                           const long* __restrict__ cptr, const int* __restrict__ citems,
                                                           const float* __restrict__ cw, long n, float* __restrict__ scores,
                                                           int* __restrict__ qsel) {
    __shared__ int r_it[PT_D * CSR_ROWS];
    __shared__ float r_w[PT_D * CSR_ROWS];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * CSR_ROWS + tid;
    CsrRow<PT_D, true> R{citems, cw, r_it, r_w, tid};
    R.stage(cptr, row, n);
    const long nc2 = pt_row_norm2(R);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    R.each_space([&](auto V) {
        for (int f = f_lo; f < f_hi; ++f) {
            if (blockIdx.x == 0 && tid == 0) qsel[f] = f;
            const double s = pt_pair(qptr, qitems, qw, f, V, nc2);
            if (row < n) scores[(size_t)f * n + row] = (float)s;
        }
    });
}

__global__ __launch_bounds__(CSR_ROWS) void k_ptype_bands(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                          const float* __restrict__ qw, int nq, int q_per,
                                                          const long* __restrict__ cptr, const int* __restrict__ citems,
                                                          const float* __restrict__ cw, long n, const BandEdges E, int nb,
                                                          long id_offset, unsigned long long* __restrict__ counts,
                                                          unsigned long long* __restrict__ first_out) {
    __shared__ int r_it[PT_D * CSR_ROWS];
    __shared__ float r_w[PT_D * CSR_ROWS];
    __shared__ BandWords s_tot;
    const int tid = threadIdx.x;
    const long row0 = (long)blockIdx.x * CSR_ROWS, row = row0 + tid;
    CsrRow<PT_D, true> R{citems, cw, r_it, r_w, tid};
    R.stage(cptr, row, n);
    const long nc2 = pt_row_norm2(R);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    for (int f0 = f_lo; f0 < f_hi; f0 += BD_QRUN) {              // workgroup-uniform: band_flush's barriers are met by all
        const int fe = f0 + BD_QRUN < f_hi ? f0 + BD_QRUN : f_hi;
        R.each_space([&](auto V) {
            for (int f = f0; f < fe; ++f) band_ballot(s_tot, f - f0, row < n, pt_pair(qptr, qitems, qw, f, V, nc2), E, nb);
        });
        band_flush(s_tot, f0, fe, nb, row0, id_offset, counts, first_out);
    }
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
        if (j < K) {
            const long id = I[(size_t)i * K + j];
            const unsigned long r = (unsigned long)id - (unsigned long)id_offset;
            if (id != -1 && r < (unsigned long)n) {
                c0 = cptr[r];
                len = csr_len(c0, cptr[r + 1]);
            } else if (id != -1) {
                bad = true;
            }
        }
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
static int tbag_args_ok(const char* what, const void* sess_ptr, const void* is_search, const void* item_id, long S, const void* item_type,
                        long n_items, long n_types, const void* err) {
    if (S <= 0 || S >= (1L << 31) || n_items <= 0 || n_items > 0x7fffffffL || n_types <= 0 || n_types > 0x7fffffffL) {
        set_error("%s: need 0 < n_sessions < 2^31, 0 < n_items < 2^31, 0 < n_types < 2^31", what);
        return SSS_EINVAL;
    }
    if (!sess_ptr || !is_search || !item_id || !item_type || !err) {
        set_error("%s: a null pointer (sess_ptr, is_search, item_id, item_type and err are required)", what);
        return SSS_EINVAL;
    }
    return SSS_OK;
}

extern "C" int sss_type_bags_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                   const int32_t* item_type, int64_t n_items, int64_t n_types, int32_t* counts, int32_t* err,
                                   void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = tbag_args_ok("type_bags_count", sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, err);
    if (rc) return rc;
    if (!counts) { set_error("type_bags_count: a null pointer (counts is required)"); return SSS_EINVAL; }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("type_bags_count: memset failed"); return SSS_EHIP; }
    const unsigned nb = (unsigned)((n_sessions * 64 + 255) / 256);
    hipLaunchKernelGGL(k_tbag_count, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, counts,
                       err);
    return check_launch("k_tbag_count");
}

extern "C" int sss_type_bags_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                  const int32_t* item_type, int64_t n_items, int64_t n_types, const int64_t* ptr, int32_t* items,
                                  float* weights, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = tbag_args_ok("type_bags_fill", sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, err);
    if (rc) return rc;
    if (!ptr || !items || !weights) { set_error("type_bags_fill: a null pointer (ptr, items and weights are required)"); return SSS_EINVAL; }
    const unsigned nb = (unsigned)((n_sessions * 64 + 255) / 256);
    hipLaunchKernelGGL(k_tbag_fill, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, item_type, n_items, n_types, ptr,
                       items, weights, err);
    return check_launch("k_tbag_fill");
}

static int pt_bags_ok(const char* what, const void* q_ptr, const void* q_items, const void* q_weights, long nq, long nq_max,
                      const void* c_ptr, const void* c_items, const void* c_weights, long n) {
    if (nq <= 0 || nq > nq_max || n <= 0 || n >= (1L << 31)) {
        if (nq_max == 65535) set_error("%s: need 0 < nq <= 65535, 0 < n < 2^31", what);
        else set_error("%s: need 0 < nq < 2^31, 0 < n < 2^31", what);
        return SSS_EINVAL;
    }
    if (!q_ptr || !q_items || !q_weights || !c_ptr || !c_items || !c_weights) {
        set_error("%s: a null pointer (both bags' ptr, items and weights are required)", what);
        return SSS_EINVAL;
    }
    return SSS_OK;
}

extern "C" size_t sss_ptype_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

extern "C" int sss_ptype_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                              const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                              int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = pt_bags_ok("ptype_topk", q_ptr, q_items, q_weights, nq, 65535, c_ptr, c_items, c_weights, n);
    if (rc) return rc;
    if (k <= 0 || k > PT_MAX_K) { set_error("ptype_topk: need 0 < k <= 1024"); return SSS_EINVAL; }
    if (!D_out || !I_out || !workspace) {
        set_error("ptype_topk: a null pointer (D_out, I_out and the workspace are required)");
        return SSS_EINVAL;
    }
    ScoreWs w;
    rc = score_ws_carve("ptype_topk", workspace, workspace_bytes, nq, n, &w);
    if (rc) return rc;
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_ptype_scores, grid, dim3(CSR_ROWS), 0, st, q_ptr, q_items, q_weights, (int)nq, q_per, c_ptr, c_items, c_weights, n,
                       w.scores, w.qsel);
    return scores_topk("k_ptype_scores", w, nq, n, k, id_offset, D_out, I_out, st);
}

extern "C" int sss_ptype_bands(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                               const int32_t* c_items, const float* c_weights, int64_t n, const double* edges, int n_edges,
                               int64_t id_offset, int64_t* counts, int64_t* first, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = pt_bags_ok("ptype_bands", q_ptr, q_items, q_weights, nq, 65535, c_ptr, c_items, c_weights, n);
    if (rc) return rc;
    BandEdges E;
    rc = band_args("ptype_bands", edges, n_edges, id_offset, nq, n, counts, first, &E, st);
    if (rc) return rc;
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_ptype_bands, grid, dim3(CSR_ROWS), 0, st, q_ptr, q_items, q_weights, (int)nq, q_per, c_ptr, c_items, c_weights, n, E,
                       n_edges + 1, id_offset, reinterpret_cast<unsigned long long*>(counts), reinterpret_cast<unsigned long long*>(first));
    return check_launch("k_ptype_bands");
}

extern "C" int sss_ptype_pair_scores(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                                     const int32_t* c_items, const float* c_weights, int64_t n, const int64_t* I, int K, int64_t id_offset,
                                     double* scores, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = pt_bags_ok("ptype_pair_scores", q_ptr, q_items, q_weights, nq, (1L << 31) - 1, c_ptr, c_items, c_weights, n);
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
