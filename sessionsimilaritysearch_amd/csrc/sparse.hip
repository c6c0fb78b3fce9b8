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
//   k_svec_count / k_svec_fill         one wave per session: item actions compacted onto the lanes, "seen before" and
//                                      ranks by readlane broadcasts (as graphbuild.hip), float64 weights
//   k_sparse_scores                    one thread per corpus row: the walk of csr_walk.h, stores coalesced across rows
//   topk_of_scores (exhaustive.hip)    the exact top-k of the score matrix, shared with the dense exhaustive search
#include <math.h>

#include "csr_walk.h"
#include "scan.h"

namespace sss {

constexpr int SV_MAX_ITEMS = 64;      // item actions per session (one lane each)
constexpr int SP_MAX_K = 1024;        // k_topk_radix's RS_MAX_K

struct InvSqrtTable { float v[SV_MAX_ITEMS + 1]; };   // v[m] = float(1 / sqrt(double(m))), made on the host

__device__ __forceinline__ double readlane_f64(double x, int lane) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

struct SessionLane {
    int m;             // distinct items of the session (0 for a flagged session)
    bool first;        // this lane holds the first occurrence of its item
    int item, rank;    // ... that item and its position in ascending item order
    double u;          // stan: sum over the item's occurrences of exp((i - L) / lammy), added in action order
    unsigned long long fm;
};

// Lane t of the wave <- the t-th item action of session s (searches skipped; `slot`: 64 ints of LDS owned by the wave).
// err bit 0: more than 64 item actions (or a decreasing sess_ptr); bit 1: an item id outside [0, n_items).  A flagged
// session counts as empty, in the count and in the fill alike, so every write stays inside the session's own range.
__device__ __forceinline__ SessionLane session_lane(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                    const long* __restrict__ item_id, long s, int t, long n_items, int stan,
                                                    double lammy, volatile int* slot, int* __restrict__ err) {
    SessionLane S;
    const long a0 = sess_ptr[s], a1 = sess_ptr[s + 1];
    const unsigned long long lt = t == 0 ? 0ull : (~0ull >> (64 - t));
    int L = 0;
    bool bad = false;
    for (long base = a0; base < a1; base += 64) {                // wave-uniform trip count
        const long a = base + t;
        const bool clk = a < a1 && is_search[a] == 0;
        const long it = clk ? item_id[a] : 0;
        const unsigned long long cm = __builtin_amdgcn_ballot_w64(clk);
        const int dest = L + __builtin_popcountll(cm & lt);
        if (clk) {
            if (it < 0 || it >= n_items) bad = true;
            if (dest < SV_MAX_ITEMS) slot[dest] = (int)it;
        }
        L += __builtin_popcountll(cm);
    }
    __builtin_amdgcn_wave_barrier();
    int flags = (L > SV_MAX_ITEMS || a1 < a0) ? 1 : 0;
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull) flags |= 2;
    if (flags) {
        if (t == 0) atomicOr(err, flags);
        L = 0;
    }
    const bool valid = t < L;
    S.item = valid ? slot[t] : -1;
    __builtin_amdgcn_wave_barrier();
    const double w = (valid && stan) ? exp((double)(t - L) / lammy) : 0.0;
    bool seen = false;
    S.u = 0.0;
    for (int u = 0; u < L; ++u) {                                // uniform loop: broadcast item action u
        const int iu = __builtin_amdgcn_readlane(S.item, u);
        const double wu = stan ? readlane_f64(w, u) : 0.0;
        if (valid && iu == S.item) {
            if (u < t) seen = true;
            S.u += wu;
        }
    }
    S.first = valid && !seen;
    S.fm = __builtin_amdgcn_ballot_w64(S.first);
    S.m = __builtin_popcountll(S.fm);
    S.rank = 0;
    for (unsigned long long todo = S.fm; todo; todo &= todo - 1) {
        const int iu = __builtin_amdgcn_readlane(S.item, __builtin_ctzll(todo));
        if (S.first && iu < S.item) ++S.rank;
    }
    return S;
}

__global__ __launch_bounds__(256) void k_svec_count(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                    const long* __restrict__ item_id, long S, long n_items,
                                                    int* __restrict__ counts, int* __restrict__ err) {
    __shared__ int slots[4 * SV_MAX_ITEMS];
    const long s = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int t = threadIdx.x & 63;
    if (s >= S) return;                                          // whole wave
    const SessionLane Ln = session_lane(sess_ptr, is_search, item_id, s, t, n_items, 0, 1.0, slots + (threadIdx.x >> 6) * SV_MAX_ITEMS, err);
    if (t == 0) counts[s] = Ln.m;
}

__global__ __launch_bounds__(256) void k_svec_fill(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                   const long* __restrict__ item_id, long S, long n_items, int stan, double lammy,
                                                   const InvSqrtTable tab, const long* __restrict__ ptr, int* __restrict__ items,
                                                   float* __restrict__ weights, int* __restrict__ err) {
    __shared__ int slots[4 * SV_MAX_ITEMS];
    const long s = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int t = threadIdx.x & 63;
    if (s >= S) return;
    const SessionLane Ln = session_lane(sess_ptr, is_search, item_id, s, t, n_items, stan, lammy, slots + (threadIdx.x >> 6) * SV_MAX_ITEMS, err);
    float w = tab.v[Ln.m];
    if (stan) {
        double ss = 0.0;                                         // sum of u^2 in ascending item order
        for (int r = 0; r < Ln.m; ++r) {
            const unsigned long long who = __builtin_amdgcn_ballot_w64(Ln.first && Ln.rank == r);
            const double ur = readlane_f64(Ln.u, __builtin_ctzll(who));
            ss += ur * ur;
        }
        w = (float)__ddiv_rn(Ln.u, __dsqrt_rn(ss));
    }
    if (Ln.first) {
        const long at = ptr[s] + Ln.rank;
        items[at] = Ln.item;
        weights[at] = w;
    }
}

// ---- scores[f][row] = float32( sum over shared items, ascending, of (double)wq * (double)wc ), accumulated in float64.
// The walk of csr_walk.h over (item, weight) entries, SP_RL of a row staged.  grid (row blocks, query ranges); block (0, y)
// also writes the identity query selection the top-k reads.
constexpr int SP_RL = 16;

__global__ __launch_bounds__(CSR_ROWS) void k_sparse_scores(const long* __restrict__ qptr, const int* __restrict__ qitems,
                                                            const float* __restrict__ qw, int nq, int q_per,
                                                            const long* __restrict__ cptr, const int* __restrict__ citems,
                                                            const float* __restrict__ cw, long n, float* __restrict__ scores,
                                                            int* __restrict__ qsel) {
    __shared__ int r_it[SP_RL * CSR_ROWS];
    __shared__ float r_w[SP_RL * CSR_ROWS];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * CSR_ROWS + tid;
    CsrRow<SP_RL, true> R{citems, cw, r_it, r_w, tid};
    R.stage(cptr, row, n);
    const int f_lo = blockIdx.y * q_per, f_hi = f_lo + q_per < nq ? f_lo + q_per : nq;
    R.each_space([&](auto V) {
        for (int f = f_lo; f < f_hi; ++f) {
            if (blockIdx.x == 0 && tid == 0) qsel[f] = f;
            const long q0 = qptr[f], q1 = q0 + csr_len(q0, qptr[f + 1]);
            double acc = 0.0;
            csr_merge(qitems, q0, q1, V, [&](long p, int j) { acc += (double)qw[p] * (double)V.weight(j); });
            if (row < n) scores[(size_t)f * n + row] = (float)acc;
        }
    });
}

// ------------------------------------------------------------------------------ host launchers
static int session_args_ok(const char* what, const void* sess_ptr, const void* is_search, const void* item_id, long S, long n_items,
                           const void* err) {
    if (S <= 0 || S >= (1L << 31) || n_items <= 0 || n_items > 0x7fffffffL || !sess_ptr || !is_search || !item_id || !err) {
        set_error("%s: need 0 < n_sessions < 2^31, 0 < n_items < 2^31, sess_ptr, is_search, item_id and err", what);
        return SSS_EINVAL;
    }
    return SSS_OK;
}

extern "C" int sss_session_vectors_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                         int64_t n_items, int32_t* counts, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = session_args_ok("session_vectors_count", sess_ptr, is_search, item_id, n_sessions, n_items, err);
    if (rc) return rc;
    if (!counts) { set_error("session_vectors_count: counts is required"); return SSS_EINVAL; }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("session_vectors_count: memset failed"); return SSS_EHIP; }
    const unsigned nb = (unsigned)((n_sessions * 64 + 255) / 256);
    hipLaunchKernelGGL(k_svec_count, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, n_items, counts, err);
    return check_launch("k_svec_count");
}

extern "C" int sss_session_vectors_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                                        int64_t n_items, int mode, double lammy, const int64_t* ptr, int32_t* items, float* weights,
                                        int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = session_args_ok("session_vectors_fill", sess_ptr, is_search, item_id, n_sessions, n_items, err);
    if (rc) return rc;
    if ((mode != 0 && mode != 1) || (mode == 1 && !(lammy > 0.0 && lammy <= 1.7976931348623157e308))) {
        set_error("session_vectors_fill: mode is 0 (binary) or 1 (stan, with a finite lammy > 0)");
        return SSS_EINVAL;
    }
    if (!ptr || !items || !weights) { set_error("session_vectors_fill: ptr, items and weights are required"); return SSS_EINVAL; }
    InvSqrtTable tab;
    tab.v[0] = 0.f;
    for (int m = 1; m <= SV_MAX_ITEMS; ++m) tab.v[m] = (float)(1.0 / sqrt((double)m));
    const unsigned nb = (unsigned)((n_sessions * 64 + 255) / 256);
    hipLaunchKernelGGL(k_svec_fill, dim3(nb), dim3(256), 0, st, sess_ptr, is_search, item_id, n_sessions, n_items, mode, lammy, tab, ptr, items,
                       weights, err);
    return check_launch("k_svec_fill");
}

// ---- the host pieces declared in csr_walk.h (jaccard.hip's entry points use them too)
static size_t ws_scores_bytes(long nq, long n) { return ((size_t)nq * n * 4 + 255) & ~(size_t)255; }
static size_t ws_qsel_bytes(long nq) { return ((size_t)nq * 4 + 255) & ~(size_t)255; }

size_t score_ws_bytes(long nq, long n) {
    if (nq <= 0 || n <= 0) return 0;
    return ws_scores_bytes(nq, n) + ws_qsel_bytes(nq) + topk_of_scores_bytes(nq, n);
}

int score_ws_carve(const char* what, void* workspace, size_t workspace_bytes, long nq, long n, ScoreWs* w) {
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("%s: workspace must be 256-byte aligned", what); return SSS_EINVAL; }
    if (workspace_bytes < score_ws_bytes(nq, n)) {
        set_error("%s: workspace %zu < %zu", what, workspace_bytes, score_ws_bytes(nq, n));
        return SSS_EWORKSPACE;
    }
    w->scores = reinterpret_cast<float*>(workspace);
    w->qsel = reinterpret_cast<int*>(reinterpret_cast<char*>(workspace) + ws_scores_bytes(nq, n));
    w->tail = reinterpret_cast<char*>(w->qsel) + ws_qsel_bytes(nq);
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

int scores_topk(const char* kernel, const ScoreWs& w, long nq, long n, int k, long id_offset, float* D_out, long* I_out, hipStream_t st) {
    const int rc = check_launch(kernel);
    if (rc) return rc;
    return topk_of_scores(w.scores, w.qsel, nq, n, k, id_offset, 0, D_out, I_out, w.tail, st);
}

extern "C" size_t sss_sparse_topk_workspace_bytes(int64_t nq, int64_t n) { return score_ws_bytes(nq, n); }

extern "C" int sss_sparse_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                               const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                               int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || n <= 0 || k <= 0 || k > SP_MAX_K || n >= (1L << 31) || nq > 65535) {
        set_error("sparse_topk: need 0 < nq <= 65535, 0 < n < 2^31, 0 < k <= 1024");
        return SSS_EINVAL;
    }
    if (!q_ptr || !q_items || !q_weights || !c_ptr || !c_items || !c_weights || !D_out || !I_out || !workspace) {
        set_error("sparse_topk: a null pointer (both CSR triples, D_out, I_out and the workspace are required)");
        return SSS_EINVAL;
    }
    ScoreWs w;
    int rc = score_ws_carve("sparse_topk", workspace, workspace_bytes, nq, n, &w);
    if (rc) return rc;
    int q_per = 0;
    const dim3 grid = csr_grid(nq, n, &q_per);
    hipLaunchKernelGGL(k_sparse_scores, grid, dim3(CSR_ROWS), 0, st, q_ptr, q_items, q_weights, (int)nq, q_per, c_ptr, c_items, c_weights,
                       n, w.scores, w.qsel);
    return scores_topk("k_sparse_scores", w, nq, n, k, id_offset, D_out, I_out, st);
}

}  // namespace sss
