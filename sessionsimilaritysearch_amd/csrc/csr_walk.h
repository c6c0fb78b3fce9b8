// Internal: the CSR row walk of the session-set kernels (k_sparse_scores in sparse.hip; k_jaccard_scores and k_jaccard_bands
// in jaccard.hip) and the host pieces of "score matrix, then exact top-k" their entry points share (defined in sparse.hip).
// overlap.hip takes csr_len only: its binary-search walk is another algorithm.
//
// THE WALK.  A thread owns one corpus row, an ascending list of distinct item ids below 2^31 - 1 (CSR_END, the sentinel).
// The first DEPTH entries of the row sit in the thread's own LDS column, [entry][thread]: the bank is the thread's,
// whatever entry each lane is at, and the thread alone reads the column back, so there is no barrier.  A wave holding a
// longer row reads its rows from global memory instead.  The query's entries are the same for the whole wave (uniform
// loads); each lane advances through its row as the query's items ascend (csr_merge).
#pragma once
#include "sss_common.h"

namespace sss {

constexpr int CSR_ROWS = 256;             // corpus rows, and threads, per workgroup
constexpr int CSR_END = 0x7fffffff;

// entries of the CSR row [a, b): 0 for a decreasing ptr, clamped to int
__host__ __device__ __forceinline__ int csr_len(long a, long b) {
    const long l = b - a;
    return l < 0 ? 0 : l > 0x7fffffffL ? 0x7fffffff : (int)l;
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

// ------------------------------------------------------------------------------ host: score matrix, then exact top-k
// Workspace: scores f32 [nq][n] | (256-byte aligned) identity query selection i32 [nq] | (aligned) the top-k's tail.
struct ScoreWs {
    float* scores;
    int* qsel;
    void* tail;
};
size_t score_ws_bytes(long nq, long n);                             // 0 unless nq > 0 and n > 0
// `workspace` carved into *w, or SSS_EINVAL / SSS_EWORKSPACE with a message that starts with `what`: it must be 256-byte
// aligned and hold score_ws_bytes(nq, n).
int score_ws_carve(const char* what, void* workspace, size_t workspace_bytes, long nq, long n, ScoreWs* w);
// grid (row blocks of CSR_ROWS, query ranges of *q_per): a small corpus splits the queries too, ~1024 workgroups
dim3 csr_grid(long nq, long n, int* q_per);
// The tail after the launch of `kernel`, which wrote w.scores and w.qsel: its launch status, then topk_of_scores (metric 0).
int scores_topk(const char* kernel, const ScoreWs& w, long nq, long n, int k, long id_offset, float* D_out, long* I_out, hipStream_t st);

}  // namespace sss
