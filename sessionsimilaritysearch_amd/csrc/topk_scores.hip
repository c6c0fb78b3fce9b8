// The exact top-k of a finished score matrix (scan.h: topk_of_scores): the tail of the dense exhaustive search
// (exhaustive.hip) and of the sparse, Jaccard and product-type indexes (csr_walk.h: score_topk).  O(n) radix selection per
// query; long rows after a multi-workgroup compaction of the rows that can still matter.  DESIGN.md "exactness".
#include "scan.h"
#include "slab_compact.h"

namespace sss {

// One block per selected query: exact top-k of its n canonical scores in O(n):
//   1. radix select (4 passes of 8 bits over the order-preserving uint of the score, LDS
//      histograms) -> T = the k-th best score and how many rows tied at T are still needed;
//   2. collect every row better than T (unordered) and, scanning ids in increasing order, the
//      lowest-id rows equal to T;
//   3. bitonic sort of the k collected (score desc, id asc) keys, write.
// Correct for any amount of ties (mass duplicates, identical rows).
constexpr int RS_THREADS = 1024;
// With a compacted input (cs != nullptr and the query's survivors fit `cap`): the select runs over the
// query's `ctotal` survivors (scores cs, row ids cids, in increasing id order) instead of all n rows.
__global__ __launch_bounds__(RS_THREADS) void k_topk_radix(const float* __restrict__ scores,
                                                           const int* __restrict__ qsel, long n_rows, int k,
                                                           long id_offset, int metric,
                                                           float* __restrict__ D_out, long* __restrict__ I_out,
                                                           const float* __restrict__ cs, const int* __restrict__ cids,
                                                           const unsigned* __restrict__ ctotal, int cap) {
    __shared__ unsigned hist[RADIX_HIST_WORDS];
    __shared__ unsigned long long keys[RS_MAX_K];
    __shared__ unsigned s_count, s_wave[RS_THREADS / 64];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const float* s = scores + (size_t)f * n_rows;
    const int* ids = nullptr;
    long n = n_rows;
    if (cs && ctotal[f] <= (unsigned)cap) { s = cs + (size_t)f * cap; ids = cids + (size_t)f * cap; n = (long)ctotal[f]; }
    const size_t out = (size_t)qsel[f] * k;
    auto key_of = [&](long i) { return f2ord(metric == 0 ? s[i] : -s[i]); };
    auto id_of = [&](long i) { return ids ? (unsigned)ids[i] : (unsigned)i; };
    const int kk = (long)k < n_rows ? k : (int)n_rows;  // rows actually returned (a compacted input holds at least kk)
    int K2 = 64;
    while (K2 < kk) K2 <<= 1;
    for (int i = tid; i < K2; i += RS_THREADS) keys[i] = 0ull;
    unsigned T = 0, need = kk;
    if (kk < n) {                                        // (kk == n: every row is returned, no selection needed)
        // the descent of block_select.h's kth_largest_of with a histogram fill of its own
        unsigned prefix = 0, mask = 0;
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            for (int i = tid; i < 256; i += RS_THREADS) hist[i] = 0;
            __syncthreads();
            // four independent loads in flight per thread (the passes are latency-bound otherwise);
            // whole waves stay in the loop so the ballots below are convergent
            const long n_up = (n + 4 * RS_THREADS - 1) / (4 * RS_THREADS) * (4 * RS_THREADS);
            for (long i0 = tid; i0 < n_up; i0 += 4 * RS_THREADS) {
                unsigned keyv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long i = i0 + (long)u * RS_THREADS;
                    keyv[u] = i < n ? key_of(i) : 0u;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const long i = i0 + (long)u * RS_THREADS;
                    const unsigned key = keyv[u];
                    const bool act = i < n && (key & mask) == prefix;
                    const unsigned b = (key >> shift) & 255u;
                    if (pass == 0) {
                        // sign and exponent bits are shared by most scores: one LDS atomic per
                        // DISTINCT bucket of the wave instead of 64 serialised ones on the same address
                        unsigned long long todo = __builtin_amdgcn_ballot_w64(act);
                        while (todo) {
                            const int leader = __builtin_ctzll(todo);
                            const unsigned lb = (unsigned)__builtin_amdgcn_readlane((int)b, leader);
                            const unsigned long long m = __builtin_amdgcn_ballot_w64(act && b == lb);
                            if (lane == leader) atomicAdd(&hist[lb], (unsigned)__builtin_popcountll(m));
                            todo &= ~m;
                        }
                    } else if (act) {
                        atomicAdd(&hist[b], 1u);
                    }
                }
            }
            __syncthreads();
            if (tid < 64) radix_pick_bin(hist, need, tid);
            __syncthreads();
            prefix |= hist[256] << shift;
            need = hist[257];                            // rank still to find inside the chosen bucket
            mask |= 255u << shift;
            __syncthreads();
        }
        T = prefix;                                      // the kk-th best key; `need` rows equal to it are wanted
    }
    if (tid == 0) s_count = 0;
    __syncthreads();
    // ---- rows strictly better than T (fewer than kk of them), in any order
    if (kk < n) {
        for (long i0 = tid; i0 < n; i0 += 4 * RS_THREADS) {
            unsigned keyv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = i0 + (long)u * RS_THREADS;
                keyv[u] = i < n ? key_of(i) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long i = i0 + (long)u * RS_THREADS;
                if (i < n && keyv[u] > T) {
                    const unsigned p = atomicAdd(&s_count, 1u);
                    keys[p] = ((unsigned long long)keyv[u] << 32) | (unsigned)(~id_of(i));
                }
            }
        }
    }
    __syncthreads();
    // ---- rows equal to T (every row when kk == n), lowest ids first: chunks in id order, rank in thread order
    const unsigned want = kk < n ? need : (unsigned)kk;
    unsigned taken = 0;
    for (long base = 0; base < n && taken < want; base += RS_THREADS) {
        const long i = base + tid;
        unsigned key = 0;
        bool hit[1] = {false};
        if (i < n) { key = key_of(i); hit[0] = kk < n ? key == T : true; }
        block_rank<RS_THREADS, 1>(hit, s_wave, tid, [&](const unsigned (&before)[1], const unsigned (&total)[1]) {
            const unsigned rank = taken + before[0];
            if (hit[0] && rank < want) keys[s_count + rank] = ((unsigned long long)key << 32) | (unsigned)(~id_of(i));
            taken += total[0];
        });
    }
    __syncthreads();
    // ---- order by (score desc, id asc) == key descending; padding keys are 0
    sort_keys<RS_THREADS, true>(keys, K2, tid);
    for (int i = tid; i < k; i += RS_THREADS) {
        if (i < kk) {
            const float v = key_score(keys[i]);
            D_out[out + i] = metric == 0 ? v : -v;
            I_out[out + i] = (long)key_id(keys[i]) + id_offset;
        } else {                                         // faiss pads missing results
            D_out[out + i] = metric == 0 ? -3.4028234663852886e38f : 3.4028234663852886e38f;
            I_out[out + i] = -1;
        }
    }
}


// ---- compaction pre-pass for long rows (n >= CP_MIN_N): the single-workgroup select above is bound by
// its own load latency (6 sweeps over n).  The kk-th best key of CP_HEAD evenly spread scores is a lower
// bound T0 of the true kk-th best, so every row of the answer (ties included) has key >= T0; those
// rows are compacted IN ID ORDER by many workgroups (slab_compact.h under KeepTopk) and the select
// then runs over the survivors.  More survivors than CP_CAP (rows sorted ascending, say): the select
// falls back to the full row -- speed only, never correctness.
constexpr int CP_HEAD = 32768;        // sampled scores (their ordinals are staged in 128 KB of LDS: one fetch, four radix passes)
constexpr int CP_SLAB = 65536;
constexpr int CP_CAP = 131072;
constexpr long CP_MIN_N = 262144;

__global__ __launch_bounds__(RS_THREADS) void k_head_threshold(const float* __restrict__ scores, long n, int k, int metric,
                                                               unsigned* __restrict__ T0) {
    extern __shared__ __attribute__((aligned(16))) unsigned ords[];     // [head] ordinals of the sampled scores
    __shared__ unsigned hist[RADIX_HIST_WORDS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const float* s = scores + (size_t)f * n;
    const long head = n < CP_HEAD ? n : CP_HEAD;         // sample size; rows i * stride: an evenly spread sample
    const long stride = n / head;                        // (corpora are often ordered -- by session length, by prefix ...)
    // The sample is fetched ONCE (every element its own cache line: with the four passes reading global memory this single
    // workgroup spent 0.40 ms per query on 262 k scattered loads at 4M rows).  k <= 1024 (always, on the paths that reach
    // this kernel today): a thread keeps only the MAXIMUM of its 32 samples -- 1024 distinct rows, so their k-th largest is
    // still a value that k rows reach -- and the radix passes run over 1024 words instead of 32768 (the first pass of the
    // full form put all 32768 LDS atomics on two or three bins: 0.23 ms per query even from LDS).  The bound is a little
    // looser (about the top 2 % of the corpus survive the compaction instead of 1.5 %).
    const int need = (int)((long)k < head ? k : head);
    int cnt = (int)head;
    if (need <= RS_THREADS && head >= RS_THREADS) {
        unsigned best = 0u;
        for (long i = tid; i < head; i += RS_THREADS) {
            const float v = s[i * stride];
            best = max(best, f2ord(metric == 0 ? v : -v));
        }
        ords[tid] = best;
        cnt = RS_THREADS;
    } else {
        for (long i = tid; i < head; i += RS_THREADS) {
            const float v = s[i * stride];
            ords[i] = f2ord(metric == 0 ? v : -v);
        }
    }
    const unsigned t0 = kth_largest_of<RS_THREADS>([&](int x) { return ords[x]; }, cnt, need, tid, hist);
    if (tid == 0) T0[f] = t0;
}

// THE TOP-K KEEP: rows with key > T0 (flag 0) and with key == T0 (flag 1).  Of the rows EQUAL to T0 only the kk lowest ids
// can ever be needed (the true kk-th best is >= T0; if it is T0 the answer takes the lowest ids among its ties), so a
// boundary inside a huge group of identical rows still compacts.  A kept row goes to cs / cids of its query at
// (#greater before) + min(#equal before, kk): ids ascending.  A query with more than `cap` kept rows is not compacted:
// the select reads its full row.
struct KeepTopk {
    static constexpr int F = 2, SLAB = CP_SLAB, COUNT_THREADS = 256, COMPACT_THREADS = RS_THREADS;
    const float* scores;
    long n;
    int k, metric;
    const unsigned* T0;
    const unsigned* total;
    int cap;
    float* cs;
    int* cids;
    unsigned t0;
    size_t out;
    __device__ unsigned kk() const { return (unsigned)((long)k < n ? k : n); }
    __device__ void load(int f) { t0 = T0[f]; out = (size_t)f * cap; }
    __device__ bool open(int f) const { return total[f] <= (unsigned)cap; }
    __device__ void classify(float v, bool (&flag)[2]) const {
        const unsigned key = f2ord(metric == 0 ? v : -v);
        flag[0] = key > t0; flag[1] = key == t0;
    }
    __device__ void emit(const bool (&flag)[2], const unsigned (&before)[2], float v, long row) const {
        if (flag[0] || (flag[1] && before[1] < kk())) {
            const size_t pos = out + before[0] + (before[1] < kk() ? before[1] : kk());
            cs[pos] = v;
            cids[pos] = (int)row;
        }
    }
};

__global__ __launch_bounds__(256) void k_count_ge(const float* __restrict__ scores, long n, int metric,
                                                  const unsigned* __restrict__ T0, int nslabs, unsigned* __restrict__ cnt_gt,
                                                  unsigned* __restrict__ cnt_eq) {
    slab_count(KeepTopk{scores, n, 0, metric, T0}, nslabs, {cnt_gt, cnt_eq});
}

// one thread block per query: exclusive scans of its slab counts (in place) + the number of rows kept
__global__ __launch_bounds__(64) void k_scan_slabs(unsigned* __restrict__ cnt_gt, unsigned* __restrict__ cnt_eq, int nslabs,
                                                   long n, int k, unsigned* __restrict__ total) {
    const int f = blockIdx.x;
    if (threadIdx.x != 0) return;
    const unsigned kk = (unsigned)((long)k < n ? k : n);
    unsigned rg = 0, re = 0;
    for (int j = 0; j < nslabs; ++j) {
        const unsigned g = cnt_gt[(size_t)f * nslabs + j], e = cnt_eq[(size_t)f * nslabs + j];
        cnt_gt[(size_t)f * nslabs + j] = rg;
        cnt_eq[(size_t)f * nslabs + j] = re;
        rg += g; re += e;
    }
    total[f] = rg + (re < kk ? re : kk);
}

__global__ __launch_bounds__(RS_THREADS) void k_compact_ge(const float* __restrict__ scores, long n, int k, int metric,
                                                           const unsigned* __restrict__ T0, int nslabs,
                                                           const unsigned* __restrict__ off_gt, const unsigned* __restrict__ off_eq,
                                                           const unsigned* __restrict__ total, int cap, float* __restrict__ cs,
                                                           int* __restrict__ cids) {
    slab_compact(KeepTopk{scores, n, k, metric, T0, total, cap, cs, cids}, nslabs, {off_gt, off_eq});
}

size_t topk_of_scores_bytes(long nsel, long n) {
    if (n < CP_MIN_N) return 0;
    const long nslabs = (n + CP_SLAB - 1) / CP_SLAB;
    return (size_t)nsel * ((size_t)CP_CAP * 8 + (size_t)nslabs * 8 + 8) + 1024;
}

// The exact top-k of a finished score matrix: scores f32 [nsel][n] -> D_out / I_out rows qsel[f], by (score desc, id asc)
// for metric 0 ((distance asc, id asc) for metric 1), ids = row + id_offset, padding beyond n.  Long rows are compacted
// first (above).  `tail`: topk_of_scores_bytes(nsel, n) bytes, 256-byte aligned.  nsel <= 65535, n < 2^31, k <= RS_MAX_K
// are the callers' to check.
int topk_of_scores(const float* scores, const int* qsel, long nsel, long n, int k, long id_offset, int metric, float* D_out,
                   long* I_out, void* tail, hipStream_t st) {
    int rc;
    const float* cs = nullptr; const int* cids = nullptr; const unsigned* ctotal = nullptr;
    if (n >= CP_MIN_N) {
        const int nslabs = (int)((n + CP_SLAB - 1) / CP_SLAB);
        char* p = reinterpret_cast<char*>(tail);
        float* cs_w = reinterpret_cast<float*>(p);                       p += (size_t)nsel * CP_CAP * 4;
        int* cids_w = reinterpret_cast<int*>(p);                         p += (size_t)nsel * CP_CAP * 4;
        unsigned* cnt_gt = reinterpret_cast<unsigned*>(p);               p += (size_t)nsel * nslabs * 4;
        unsigned* cnt_eq = reinterpret_cast<unsigned*>(p);               p += (size_t)nsel * nslabs * 4;
        unsigned* T0 = reinterpret_cast<unsigned*>(p);                   p += (size_t)nsel * 4;
        unsigned* total = reinterpret_cast<unsigned*>(p);
        rc = opt_in_lds(reinterpret_cast<const void*>(&k_head_threshold), "k_head_threshold", (size_t)CP_HEAD * 4);
        if (rc) return rc;
        hipLaunchKernelGGL(k_head_threshold, dim3((unsigned)nsel), dim3(RS_THREADS), (size_t)CP_HEAD * 4, st, scores, n, k, metric, T0);
        rc = check_launch("k_head_threshold");
        if (rc) return rc;
        hipLaunchKernelGGL(k_count_ge, dim3((unsigned)nslabs, (unsigned)nsel), dim3(256), 0, st, scores, n, metric, T0, nslabs, cnt_gt, cnt_eq);
        hipLaunchKernelGGL(k_scan_slabs, dim3((unsigned)nsel), dim3(64), 0, st, cnt_gt, cnt_eq, nslabs, n, k, total);
        hipLaunchKernelGGL(k_compact_ge, dim3((unsigned)nslabs, (unsigned)nsel), dim3(RS_THREADS), 0, st, scores, n, k, metric, T0, nslabs,
                           cnt_gt, cnt_eq, total, CP_CAP, cs_w, cids_w);
        rc = check_launch("k_compact_ge");
        if (rc) return rc;
        cs = cs_w; cids = cids_w; ctotal = total;
    }
    hipLaunchKernelGGL(k_topk_radix, dim3((unsigned)nsel), dim3(RS_THREADS), 0, st, scores, qsel, n, k, id_offset, metric, D_out, I_out,
                       cs, cids, ctotal, CP_CAP);
    return check_launch("k_topk_radix");
}

}  // namespace sss
