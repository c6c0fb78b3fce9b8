// Internal: the compaction of the rows of a [nsel][n] score matrix that a query KEEPS, in row order, by many workgroups:
// count per slab (slab_count, grid (slabs, nsel)), an exclusive scan of every query's slab counts in place (the callers'
// own few lines: k_scan_slabs, k_range_scan), ordered write at (kept rows of the earlier slabs) + (rank in thread order)
// (slab_compact, grid (slabs, nsel)).  The frame of topk_scores.hip's k_count_ge / k_compact_ge and
// range_exhaustive.hip's k_range_count / k_range_compact, which differ in what they keep and where it goes:
//
//     struct Keep {
//         static constexpr int F;                        // flags a row is classified by: a count array and a rank each
//         static constexpr int SLAB, COUNT_THREADS, COMPACT_THREADS;
//         const float* scores; long n;                   // the matrix
//         void load(int f);                              // per-query state of query f, once per workgroup
//         bool open(int f);                              // after load, slab_compact only: false = nothing of f is written
//         void classify(float score, bool (&flag)[F]) const;
//         void emit(const bool (&flag)[F], const unsigned (&before)[F], float score, long row) const;
//     };
//
// emit: before[a] = the query's rows in front of `row` with flag a set; the Keep turns that into a position, bounds it
// and writes.  cnt[a]: u32 [nsel][nslabs], counts after slab_count, offsets after the scan.
#pragma once
#include "block_select.h"

namespace sss {

template <typename Keep>
__device__ __forceinline__ void slab_count(Keep K, int nslabs, unsigned* const (&cnt)[Keep::F]) {
    constexpr int F = Keep::F, NT = Keep::COUNT_THREADS;
    __shared__ unsigned s_wave[F * NT / 64];
    const int f = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    K.load(f);
    const float* s = K.scores + (size_t)f * K.n;
    const long lo = (long)slab * Keep::SLAB, hi = lo + Keep::SLAB < K.n ? lo + Keep::SLAB : K.n;
    unsigned c[F] = {};
#pragma unroll 2                                                         // two loads in flight
    for (long i = lo + tid; i < hi; i += NT) {
        bool flag[F];
        K.classify(s[i], flag);
#pragma unroll
        for (int a = 0; a < F; ++a) c[a] += flag[a] ? 1u : 0u;
    }
    block_sum<NT, F>(c, s_wave, tid);
    if (tid == 0) {
#pragma unroll
        for (int a = 0; a < F; ++a) cnt[a][(size_t)f * nslabs + slab] = c[a];
    }
}

template <typename Keep>
__device__ __forceinline__ void slab_compact(Keep K, int nslabs, const unsigned* const (&off)[Keep::F]) {
    constexpr int F = Keep::F, NT = Keep::COMPACT_THREADS;
    __shared__ unsigned s_wave[F * NT / 64];
    const int f = blockIdx.y, slab = blockIdx.x, tid = threadIdx.x;
    K.load(f);
    if (!K.open(f)) return;                                              // (workgroup-uniform)
    const float* s = K.scores + (size_t)f * K.n;
    const long lo = (long)slab * Keep::SLAB, hi = lo + Keep::SLAB < K.n ? lo + Keep::SLAB : K.n;
    unsigned base[F];
#pragma unroll
    for (int a = 0; a < F; ++a) base[a] = off[a][(size_t)f * nslabs + slab];
    // the next step's score is in flight under this step's barriers; no fetch leaves the slab
    float v_next = lo + tid < hi ? s[lo + tid] : 0.f;
    for (long i0 = lo; i0 < hi; i0 += NT) {
        const long i = i0 + tid;
        const float v = v_next;
        if (i + NT < hi) v_next = s[i + NT];
        bool flag[F] = {};
        if (i < hi) K.classify(v, flag);
        block_rank<NT, F>(flag, s_wave, tid, [&](unsigned (&before)[F], const unsigned (&total)[F]) {
#pragma unroll
            for (int a = 0; a < F; ++a) before[a] += base[a];
            K.emit(flag, before, v, i);
#pragma unroll
            for (int a = 0; a < F; ++a) base[a] += total[a];
        });
    }
}

}  // namespace sss
