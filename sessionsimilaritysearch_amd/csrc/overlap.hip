// Scoring a search result: |Q_i & C_r| for every (query i, neighbour r = I[i, j]) pair of two batches of item sets, and
// the per-query sums the reference's metrics are means of (test_amazon_filterd.py: get_*_jaccard :286-343, get_*_recall
// :345-382, get_future_map :226-244, get_recall :443-450; fine_tune_ours.py: get_score / get_ave_score :42-97).
// C ABI: include/sss_eval.h; contract: DESIGN.md "Scoring a result".
//
// An item set is the (ptr, items) half of a session-vector CSR triple: ascending, distinct int32 ids.
//
//   k_item_overlap      one wave per query; the query's row staged in LDS (up to OV_QCAP items, beyond that it is
//                       searched where it lies); lane l owns the neighbours j = l, l + 64, ...: it walks the neighbour's
//                       row and binary-searches every item in the query's.  A row longer than OV_LONG is left to the
//                       whole wave afterwards (64 items a step, the hits counted by ballot), as the sparse scorer leaves
//                       its long rows to the global-memory walk: one long session must not hold 63 lanes idle.  Every
//                       (i, j) has one owner; the only atomic is the OR into err.
//   k_overlap_metrics   one thread per query, float64 sums in ascending j (the canonical order); [64 queries x 32
//                       neighbours] tiles pass through LDS so that the global reads are whole lines and the walk is
//                       conflict-free (row stride 33).
#include "csr_walk.h"

namespace sss {

constexpr int OV_WAVES = 4;           // queries per workgroup
constexpr int OV_QCAP = 2048;         // query items staged per wave: 8 KiB, 32 KiB a workgroup, five workgroups a CU
constexpr int OV_LONG = 64;           // neighbour rows longer than this are walked by the whole wave
constexpr int OV_MAX_K = 1024;

__device__ __forceinline__ long readlane_i64(long x, int lane) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long)x, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long)x >> 32), lane);
    return (long)(((unsigned long)hi << 32) | lo);
}

__global__ __launch_bounds__(OV_WAVES * 64) void k_item_overlap(const long* __restrict__ qptr, const int* __restrict__ qitems, long nq,
                                                               const long* __restrict__ cptr, const int* __restrict__ citems, long n,
                                                               const long* __restrict__ I, int K, long id_offset,
                                                               int* __restrict__ inter, int* __restrict__ csize, int* __restrict__ err) {
    __shared__ int qrow[OV_WAVES * OV_QCAP];
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * OV_WAVES + (threadIdx.x >> 6);
    int* mine = qrow + (threadIdx.x >> 6) * OV_QCAP;
    long q0 = 0;
    int ql = 0;
    if (i < nq) {
        q0 = qptr[i];
        ql = csr_len(q0, qptr[i + 1]);
    }
    const bool staged = ql <= OV_QCAP;                               // wave-uniform
    if (staged)
        for (int p = lane; p < ql; p += 64) mine[p] = qitems[q0 + p];
    __syncthreads();
    if (i >= nq) return;                                             // whole wave; no barrier below

    // One address space per instantiation (an LDS or a global row), as in k_sparse_scores: a per-lane choice would
    // turn every probe into a flat load.
    auto run = [&](auto q_at) {
        auto has = [&](int x) {                                      // x in the query's row?
            int lo = 0, hi = ql;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (q_at(mid) < x) lo = mid + 1; else hi = mid;
            }
            return lo < ql && q_at(lo) == x;
        };
        bool bad = false;
        for (int jb = 0; jb < K; jb += 64) {                         // wave-uniform trip count
            const int j = jb + lane;
            long c0 = 0;
            int len = -1, cnt = 0;
            if (j < K) len = csr_neighbour(cptr, n, I[(size_t)i * K + j], id_offset, &c0, &bad);
            if (len <= OV_LONG && ql > 0)
                for (int e = 0; e < len; ++e) cnt += has(citems[c0 + e]) ? 1 : 0;
            for (unsigned long long todo = __builtin_amdgcn_ballot_w64(len > OV_LONG && ql > 0); todo; todo &= todo - 1) {
                const int b = __builtin_ctzll(todo);                 // the owner of a long row: the whole wave walks it
                const long c0b = readlane_i64(c0, b);
                const int lenb = __builtin_amdgcn_readlane(len, b);
                int tot = 0;
                for (int e0 = 0; e0 < lenb; e0 += 64) {
                    const int e = e0 + lane;
                    const bool hit = e < lenb && has(citems[c0b + e]);
                    tot += __builtin_popcountll(__builtin_amdgcn_ballot_w64(hit));
                }
                if (lane == b) cnt = tot;
            }
            if (j < K) {
                inter[(size_t)i * K + j] = cnt;
                csize[(size_t)i * K + j] = len;
            }
        }
        if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) atomicOr(err, 1);
    };
    if (staged)
        run([&](int p) { return mine[p]; });
    else
        run([&](int p) { return qitems[q0 + p]; });
}

constexpr int OM_Q = 64;              // queries per workgroup (one thread each)
constexpr int OM_J = 32;              // neighbours per tile

__global__ __launch_bounds__(OM_Q) void k_overlap_metrics(const int* __restrict__ inter, const int* __restrict__ csize,
                                                          const int* __restrict__ qsize, long nq, int K, float thr,
                                                          double* __restrict__ out, int* __restrict__ flags) {
    __shared__ int s_in[OM_Q * (OM_J + 1)];
    __shared__ int s_cs[OM_Q * (OM_J + 1)];
    const int t = threadIdx.x;
    const long qb = (long)blockIdx.x * OM_Q, i = qb + t;
    const int qs = i < nq ? qsize[i] : 0;
    double jac = 0.0, rec = 0.0, ap = 0.0;
    int h = 0, above = 0, fl = qs == 0 ? 2 : 0;
    for (int j0 = 0; j0 < K; j0 += OM_J) {
        const int w = K - j0 < OM_J ? K - j0 : OM_J;
        __syncthreads();
        for (int e = t; e < OM_Q * OM_J; e += OM_Q) {
            const int r = e / OM_J, c = e % OM_J;
            if (qb + r < nq && c < w) {
                const size_t g = (size_t)(qb + r) * K + j0 + c;
                s_in[r * (OM_J + 1) + c] = inter[g];
                s_cs[r * (OM_J + 1) + c] = csize[g];
            }
        }
        __syncthreads();
        if (i >= nq) continue;
        for (int c = 0; c < w; ++c) {                                // ascending j: the canonical order
            const int in = s_in[t * (OM_J + 1) + c], cs = s_cs[t * (OM_J + 1) + c];
            if (cs < 0) continue;                                    // a missing neighbour keeps its rank and adds nothing
            const long u = (long)qs + cs - in;
            double s = 0.0;
            if (u == 0) fl |= 1; else s = __ddiv_rn((double)in, (double)u);
            jac += s;
            if (qs > 0) rec += __ddiv_rn((double)in, (double)qs);
            if (in > 0) {
                ++h;
                ap += __ddiv_rn((double)h, (double)(j0 + c + 1));
            }
            if ((float)s > thr) ++above;
        }
    }
    if (i >= nq) return;
    out[i * 4 + 0] = jac;
    out[i * 4 + 1] = rec;
    out[i * 4 + 2] = h ? __ddiv_rn(ap, (double)h) : 0.0;
    out[i * 4 + 3] = (double)above;
    flags[i] = fl;
}

// ------------------------------------------------------------------------------ host launchers
extern "C" int sss_item_overlap(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                                int64_t n, const int64_t* I, int K, int64_t id_offset, int32_t* inter, int32_t* csize, int32_t* err,
                                void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || nq >= (1L << 31) || K <= 0 || K > OV_MAX_K || n <= 0 || n >= (1L << 31)) {
        set_error("item_overlap: need 0 < nq < 2^31, 0 < K <= 1024, 0 < n < 2^31");
        return SSS_EINVAL;
    }
    if (!q_ptr || !q_items || !c_ptr || !c_items || !I || !inter || !csize || !err) {
        set_error("item_overlap: a null pointer (both item sets, I, inter, csize and err are required)");
        return SSS_EINVAL;
    }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("item_overlap: memset failed"); return SSS_EHIP; }
    const unsigned nb = (unsigned)((nq + OV_WAVES - 1) / OV_WAVES);
    hipLaunchKernelGGL(k_item_overlap, dim3(nb), dim3(OV_WAVES * 64), 0, st, q_ptr, q_items, nq, c_ptr, c_items, n, I, K, id_offset, inter,
                       csize, err);
    return check_launch("k_item_overlap");
}

extern "C" int sss_overlap_metrics(const int32_t* inter, const int32_t* csize, const int32_t* qsize, int64_t nq, int K, float thr,
                                   double* out, int32_t* flags, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || nq >= (1L << 31) || K <= 0 || K > OV_MAX_K) {
        set_error("overlap_metrics: need 0 < nq < 2^31, 0 < K <= 1024");
        return SSS_EINVAL;
    }
    if (!inter || !csize || !qsize || !out || !flags) {
        set_error("overlap_metrics: a null pointer (inter, csize, qsize, out and flags are required)");
        return SSS_EINVAL;
    }
    const unsigned nb = (unsigned)((nq + OM_Q - 1) / OM_Q);
    hipLaunchKernelGGL(k_overlap_metrics, dim3(nb), dim3(OM_Q), 0, st, inter, csize, qsize, nq, K, thr, out, flags);
    return check_launch("k_overlap_metrics");
}

}  // namespace sss
