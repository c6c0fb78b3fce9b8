// Internal: the CSR row walk of the exact indexes over CSR rows and the one frame their score kernels share.  The kinds are
// sparse.hip's (k_sparse_scores), jaccard.hip's (k_jaccard_scores, k_jaccard_bands) and ptype.hip's (k_ptype_scores,
// k_ptype_bands); the band kernels' frame is band_count.h's.  Also here: the decode of a neighbour id (k_ptype_pair_scores,
// overlap.hip's k_item_overlap -- whose binary-search walk is another algorithm) and the host pieces of "check, score
// matrix, exact top-k" behind the three *_topk entry points (defined in sparse.hip).
//
// THE WALK.  A thread owns one corpus row, an ascending list of distinct item ids below 2^31 - 1 (CSR_END, the sentinel).
// The first DEPTH entries of the row sit in the thread's own LDS column, [entry][thread]: the bank is the thread's,
// whatever entry each lane is at, and the thread alone reads the column back, so there is no barrier.  A wave holding a
// longer row reads its rows from global memory instead.  The query's entries are the same for the whole wave (uniform
// loads); each lane advances through its row as the query's items ascend (csr_merge).
//
// A KIND is what turns one (query, row) pair into a float64 score -- the only thing the kernels of a family differ in:
//
//     struct Kind {
//         static constexpr int DEPTH;         // entries of a row staged in LDS
//         static constexpr bool WEIGHTS;      // ... with their weights (then 8 bytes an entry)
//         static State row_state(const CsrRow<DEPTH, WEIGHTS>&);      // taken once after staging; NoRowState: nothing
//         template <class View> static double pair(const CsrSets& Q, long q0, int ql, const View& V, State);
//     };
//
// pair: the score of the ql query entries of Q from q0 on against the thread's row on the view V (V.lr: the row's length).
// csr_scores stores (float)pair(...); band_count.h's csr_bands ballots pair(...) itself.
#pragma once
#include "sss_common.h"

namespace sss {

constexpr int CSR_ROWS = 256;             // corpus rows, and threads, per workgroup
constexpr int CSR_END = 0x7fffffff;
constexpr int CSR_LDS_WORDS = 32768 / 4;  // the staged rows of a workgroup: items, then weights where a kind reads them

// A batch of CSR rows: ptr [rows + 1], items, and the weights (null where the kind reads none).
struct CsrSets {
    const long* ptr;
    const int* items;
    const float* w;
};

// entries of the CSR row [a, b): 0 for a decreasing ptr, clamped to int
__host__ __device__ __forceinline__ int csr_len(long a, long b) {
    const long l = b - a;
    return l < 0 ? 0 : l > 0x7fffffffL ? 0x7fffffff : (int)l;
}

// The row of the neighbour `id` (an entry of a result I) in a corpus of n rows whose ids start at id_offset: its length,
// with *c0 its first entry; -1 and *c0 untouched for the padding id -1 and for any other id outside the corpus, which
// sets *bad as well.
__device__ __forceinline__ int csr_neighbour(const long* __restrict__ cptr, long n, long id, long id_offset, long* c0, bool* bad) {
    const unsigned long r = (unsigned long)id - (unsigned long)id_offset;
    if (id != -1 && r < (unsigned long)n) {
        *c0 = cptr[r];
        return csr_len(*c0, cptr[r + 1]);
    }
    if (id != -1) *bad = true;
    return -1;
}

// One address space of a staged row: its length, its first item (or the sentinel) and its accessors.
template <class ItemAt, class WeightAt>
struct CsrView {
    int lr, first;
    ItemAt item;
    WeightAt weight;
};

// The thread's row.  s_it / s_w: the workgroup's LDS columns, int / float [DEPTH * CSR_ROWS]; cw and s_w are null when
// WEIGHTS is false, and then no view's weight() may be called.  32 KiB a workgroup either way.
template <int DEPTH, bool WEIGHTS>
struct CsrRow {
    static_assert(DEPTH * CSR_ROWS * (WEIGHTS ? 8 : 4) == 32768, "the staged rows take 32 KiB a workgroup");
    const int* citems;
    const float* cw;
    int* s_it;
    float* s_w;
    int tid;
    long r0 = 0;              // the row's first entry in citems
    int lr = 0;               // its length (0 beyond the corpus)
    bool wave_long = false;   // some row of this wave is longer than its LDS column

    __device__ __forceinline__ void stage(const long* __restrict__ cptr, long row, long n) {
        if (row < n) {
            r0 = cptr[row];
            lr = csr_len(r0, cptr[row + 1]);
        }
        for (int j = 0; j < DEPTH && j < lr; ++j) {
            s_it[j * CSR_ROWS + tid] = citems[r0 + j];
            if constexpr (WEIGHTS) s_w[j * CSR_ROWS + tid] = cw[r0 + j];
        }
        wave_long = __builtin_amdgcn_ballot_w64(lr > DEPTH) != 0ull;
    }

    // run(view) on the form the wave takes: every row of the wave fits its LDS column (ds_read only), or some row is
    // longer and the whole wave reads its rows from global memory.  `run` is instantiated once per form, so each of its
    // loops sees ONE address space -- a per-lane choice between an LDS and a global address would turn every step into a
    // flat load.
    template <class Run>
    __device__ __forceinline__ void each_space(Run run) const {
        auto with = [&](auto item_at, auto weight_at) {
            run(CsrView<decltype(item_at), decltype(weight_at)>{lr, lr > 0 ? item_at(0) : CSR_END, item_at, weight_at});
        };
        if (!wave_long)
            with([&](int j) { return s_it[j * CSR_ROWS + tid]; }, [&](int j) { return s_w[j * CSR_ROWS + tid]; });
        else
            with([&](int j) { return citems[r0 + j]; }, [&](int j) { return cw[r0 + j]; });
    }
};

// hit(p, j) for every item the query entries [q0, q1) share with the row, in ascending item order: p the query entry, j the
// row entry.
template <class View, class Hit>
__device__ __forceinline__ void csr_merge(const int* __restrict__ qitems, long q0, long q1, const View& V, Hit hit) {
    int j = 0, cur = V.first;
    for (long p = q0; p < q1; ++p) {
        const int qi = qitems[p];
        while (cur < qi) {
            ++j;
            cur = j < V.lr ? V.item(j) : CSR_END;
        }
        if (cur == qi && j < V.lr) hit(p, j);
    }
}

struct NoRowState {};

// The thread's row of a workgroup of a Kind's kernels, staged: `cols` is the workgroup's CSR_LDS_WORDS of LDS.
template <class Kind>
__device__ __forceinline__ CsrRow<Kind::DEPTH, Kind::WEIGHTS> csr_stage(int* cols, const CsrSets& C, long row, long n) {
    float* s_w = Kind::WEIGHTS ? reinterpret_cast<float*>(cols + Kind::DEPTH * CSR_ROWS) : nullptr;
    CsrRow<Kind::DEPTH, Kind::WEIGHTS> R{C.items, C.w, cols, s_w, (int)threadIdx.x};
    R.stage(C.ptr, row, n);
    return R;
}

// The queries [*f_lo, f_hi) of workgroup (x, y) of a csr_grid launch
__device__ __forceinline__ int csr_query_range(int nq, int q_per, int* f_lo) {
    *f_lo = blockIdx.y * q_per;
    return *f_lo + q_per < nq ? *f_lo + q_per : nq;
}

// THE SCORE FRAME: scores[f][row] = (float)Kind::pair(query f, row) for the workgroup's rows and queries.  grid: csr_grid's
// (row blocks, query ranges); block (0, y) also writes the identity query selection the top-k reads.
template <class Kind>
__device__ __forceinline__ void csr_scores(const CsrSets& Q, int nq, int q_per, const CsrSets& C, long n, float* __restrict__ scores,
                                           int* __restrict__ qsel) {
    __shared__ int cols[CSR_LDS_WORDS];
    const int tid = threadIdx.x;
    const long row = (long)blockIdx.x * CSR_ROWS + tid;
    const auto R = csr_stage<Kind>(cols, C, row, n);
    const auto state = Kind::row_state(R);
    int f_lo;
    const int f_hi = csr_query_range(nq, q_per, &f_lo);
    R.each_space([&](auto V) {
        for (int f = f_lo; f < f_hi; ++f) {
            if (blockIdx.x == 0 && tid == 0) qsel[f] = f;
            const long q0 = Q.ptr[f];
            const double s = Kind::pair(Q, q0, csr_len(q0, Q.ptr[f + 1]), V, state);
            if (row < n) scores[(size_t)f * n + row] = (float)s;
        }
    });
}

// ------------------------------------------------------------------------------ host (defined in sparse.hip)
// The CSR arguments every search entry point takes, checked: 0 < nq <= nq_max and 0 < n < 2^31, then no null ptr or items
// (or weights, when `weighted`).  SSS_OK, or SSS_EINVAL with a message that starts with `what`.
int csr_args_ok(const char* what, const CsrSets& Q, long nq, long nq_max, const CsrSets& C, long n, bool weighted);
// grid (row blocks of CSR_ROWS, query ranges of *q_per): a small corpus splits the queries too, ~1024 workgroups
dim3 csr_grid(long nq, long n, int* q_per);

// Score matrix, then exact top-k.  Workspace: scores f32 [nq][n] | (256-byte aligned) identity query selection i32 [nq] |
// (aligned) the top-k's tail.
size_t score_ws_bytes(long nq, long n);                             // 0 unless nq > 0 and n > 0
// A kind's score kernel: (qptr, qitems, qw, nq, q_per, cptr, citems, cw, n, scores, qsel), on csr_grid's grid.
using ScoreKernel = void (*)(const long*, const int*, const float*, int, int, const long*, const int*, const float*, long, float*, int*);
// A *_topk entry point: csr_args_ok, k, the remaining pointers, the workspace (256-byte aligned, score_ws_bytes(nq, n):
// SSS_EINVAL / SSS_EWORKSPACE), the launch of `kernel` (`name`), its status, then topk_of_scores (metric 0).  Messages start
// with `what`.
int score_topk(const char* what, const char* name, ScoreKernel kernel, const CsrSets& Q, long nq, const CsrSets& C, long n,
               bool weighted, int k, long id_offset, float* D_out, long* I_out, void* workspace, size_t workspace_bytes, hipStream_t st);

}  // namespace sss
