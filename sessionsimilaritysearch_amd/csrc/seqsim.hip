// The string metrics of a search result: Levenshtein.seqratio of two lists of strings and get_string_match's two counts for
// every (query i, neighbour r = I[i, j]) pair (fine_tune_ours.py: get_score 'all_query_score' / 'all_product_title_score'
// :56-65; util_amazon_filtered.py: get_string_match :239-249; test_amazon_filterd.py: get_query_metric :416-441).
// C ABI and the score of record: include/ext/sss_seqsim.h; contract and layout: DESIGN.md section 5.12.
//
//   k_seq_pair_scores   one 256-thread workgroup per session pair (a grid-stride loop over the nq * K pairs).
//                       1. the first 128 threads read the two sequences' string ids, offsets and lengths into LDS and
//                          check them against the limits: a pair that breaks one is MISSING, nothing is truncated;
//                       2. the four waves take the n1 * n2 string pairs in turn.  Equal ids cost 0 and match without any
//                          work.  Otherwise the whole wave computes one LCS with the bit-parallel recurrence
//                          V' = (V + (V & M)) | (V & ~M) over 64-bit words, the carry passed from word to word: lane l holds
//                          character 64 w + l of the string in words (a register per word), the match word M of one
//                          character of the other string against 64 of them is ONE ballot, and V, the carry and the loop
//                          are wave-uniform (scalar registers, scalar ALU).  The string whose role as the word string costs
//                          fewer steps takes it (ceil(la / 64) * lb against ceil(lb / 64) * la).  The LCS is the number of
//                          zero bits of V.  Lane 0 writes c_ij into the LDS cost matrix (doubles, 32 KiB) and the two match
//                          flags (every writer stores the same 1);
//                       3. wave 0 counts the flags by ballot and fills T along anti-diagonals, lane i - 1 owning row i: the
//                          three neighbours of a cell are the lane's own last value and two lane shifts.  Every cell is the
//                          minimum of the same three rounded sums as in the row-by-row order, so the bits are the same.
//   k_seq_query_metric  one thread per query, float64 sums in ascending j (the canonical order).
//
// What the length filter of the issue's sketch would save -- 11 min(la, lb) <= 9 max(la, lb) cannot match -- is nothing here:
// d is needed for c_ij either way, and with d in hand the match is one integer comparison.
#include "csr_walk.h"
#include "../../include/ext/sss_seqsim.h"

namespace sss {

constexpr int SQ_WAVES = 4;
constexpr int SQ_N = SSS_SEQ_MAX_STRINGS;                 // 64: one lane per row of T
constexpr int SQ_WORDS = SSS_STR_MAX_CHARS / 64;          // 16 words of 64 characters
constexpr int SQ_MAX_K = 1024;
constexpr unsigned SQ_MAX_BLOCKS = 1u << 16;
static_assert(SQ_N == 64 && SQ_WORDS * 64 == SSS_STR_MAX_CHARS, "one lane per sequence entry, whole words per string");

// A value every lane of the wave holds alike, as one the compiler knows to be wave-uniform (what it reads from LDS or
// derives from threadIdx it takes for divergent): the loops and branches on it, and the recurrence below, then run on the
// scalar unit.
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }
__device__ __forceinline__ long uniform(long x) {
    const unsigned lo = (unsigned)uniform((int)(unsigned)(unsigned long)x), hi = (unsigned)uniform((int)(unsigned)((unsigned long)x >> 32));
    return (long)(((unsigned long)hi << 32) | lo);
}

// LCS(a, b) by the whole wave; a: la <= 64 NW characters from a0 on (the word string), b: lb characters from b0 on.
// Wave-uniform arguments and result.  Lanes past la hold -1, which equals no code point: their bits of M are 0, so their
// bits of V stay 1 (a carry into them is OR-ed back by V & ~M) and are not counted.
template <int NW>
__device__ __forceinline__ int lcs_wave(const int* __restrict__ chars, long a0, int la, long b0, int lb, int lane) {
    int av[NW];
    unsigned long long V[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        av[w] = w * 64 + lane < la ? chars[a0 + w * 64 + lane] : -1;
        V[w] = ~0ull;
    }
    for (int k0 = 0; k0 < lb; k0 += 64) {
        const int bv = k0 + lane < lb ? chars[b0 + k0 + lane] : -2;
        const int kn = lb - k0 < 64 ? lb - k0 : 64;
        for (int k = 0; k < kn; ++k) {
            const int c = __builtin_amdgcn_readlane(bv, k);
            unsigned long long carry = 0ull;
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const unsigned long long M = __builtin_amdgcn_ballot_w64(av[w] == c);
                const unsigned long long u = V[w] & M;
                const unsigned long long s1 = V[w] + u;
                const unsigned long long s2 = s1 + carry;
                // the carries out of bit 63 from bit operations alone (generate | propagate & ~sum; u is a subset of V):
                // there is no scalar 64-bit "less than", and a vector compare would pull the recurrence off the scalar unit
                carry = (u | (V[w] & ~s1) | (s1 & ~s2)) >> 63;
                V[w] = s2 | (V[w] & ~M);
            }
        }
    }
    int zeros = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) zeros += __builtin_popcountll(~V[w]);
    return zeros;
}

// the instantiation for a word string of `la` characters: 1, 2, 4, 8 or 16 words
__device__ __forceinline__ int lcs_any(const int* __restrict__ chars, long a0, int la, long b0, int lb, int lane) {
    if (la <= 64) return lcs_wave<1>(chars, a0, la, b0, lb, lane);
    if (la <= 128) return lcs_wave<2>(chars, a0, la, b0, lb, lane);
    if (la <= 256) return lcs_wave<4>(chars, a0, la, b0, lb, lane);
    if (la <= 512) return lcs_wave<8>(chars, a0, la, b0, lb, lane);
    return lcs_wave<SQ_WORDS>(chars, a0, la, b0, lb, lane);
}

__global__ __launch_bounds__(SQ_WAVES * 64) void k_seq_pair_scores(const long* __restrict__ sptr, const int* __restrict__ chars, long ns,
                                                                  const long* __restrict__ qptr, const int* __restrict__ qids, long nq,
                                                                  const long* __restrict__ cptr, const int* __restrict__ cids, long n,
                                                                  const long* __restrict__ I, int K, long id_offset,
                                                                  double* __restrict__ ratio, int* __restrict__ qmatch,
                                                                  int* __restrict__ cmatch, int* __restrict__ clen, int* __restrict__ err) {
    __shared__ double cost[SQ_N * SQ_N];                   // c_ij at [i * n2 + j]
    __shared__ long s_off[2 * SQ_N];                       // first character of Q's strings, then of C's
    __shared__ int s_id[2 * SQ_N], s_len[2 * SQ_N], s_match[2 * SQ_N];
    __shared__ int s_bad;
    const int tid = threadIdx.x, lane = tid & 63, wave = uniform(tid >> 6);
    const long total = nq * K;
    for (long p = blockIdx.x; p < total; p += gridDim.x) {
        const long i = p / K;
        __syncthreads();                                             // the last pair's readers are done with the LDS
        if (tid == 0) s_bad = 0;
        __syncthreads();
        // ---- 1. the two sequences (every thread reads the four ptr words: uniform loads)
        const long q0 = qptr[i];
        const int n1 = csr_len(q0, qptr[i + 1]);
        long c0 = 0;
        bool outside = false;
        const int n2 = csr_neighbour(cptr, n, I[p], id_offset, &c0, &outside);
        int bad = outside ? 1 : 0;
        if (n2 >= 0 && (n1 > SQ_N || n2 > SQ_N)) bad |= 2;
        if (n2 >= 0 && !bad && tid < 2 * SQ_N) {
            const int e = tid & (SQ_N - 1);
            const bool mine = tid < SQ_N ? e < n1 : e < n2;
            if (mine) {
                const int id = tid < SQ_N ? qids[q0 + e] : cids[c0 + e];
                long o = 0;
                int len = 0;
                if (id < 0 || id >= ns) {
                    atomicOr(&s_bad, 2);
                } else {
                    o = sptr[id];
                    const long l = sptr[id + 1] - o;
                    if (l < 0 || l > SSS_STR_MAX_CHARS) atomicOr(&s_bad, 2); else len = (int)l;
                }
                s_id[tid] = id;
                s_off[tid] = o;
                s_len[tid] = len;
            }
            s_match[tid] = 0;
        }
        __syncthreads();
        bad = uniform(bad | s_bad);                                  // workgroup-uniform from here on
        if (n2 < 0 || bad) {
            if (tid == 0) {
                ratio[p] = __builtin_nan("");
                qmatch[p] = 0;
                cmatch[p] = 0;
                clen[p] = -1;
                if (bad) atomicOr(err, bad);
            }
            continue;
        }
        // ---- 2. the string pairs, a wave each
        for (int sp = wave; sp < n1 * n2; sp += SQ_WAVES) {
            const int a = sp / n2, b = sp - a * n2;
            int d = 0, L = 0;
            if (uniform(s_id[a]) != uniform(s_id[SQ_N + b])) {
                const int la = uniform(s_len[a]), lb = uniform(s_len[SQ_N + b]);
                const long oa = uniform(s_off[a]), ob = uniform(s_off[SQ_N + b]);
                L = la + lb;
                const bool a_words = ((la + 63) >> 6) * lb <= ((lb + 63) >> 6) * la;      // the cheaper role for a
                const int lcs = lcs_any(chars, a_words ? oa : ob, a_words ? la : lb, a_words ? ob : oa, a_words ? lb : la, lane);
                d = L - 2 * lcs;
            }
            if (lane == 0) {
#pragma clang fp contract(off)                                        // 2.0 / L rounded, then the product rounded
                cost[sp] = L == 0 ? 0.0 : (2.0 / (double)L) * (double)d;
                if (L == 0 || L > 10 * d) {                          // ratio > 0.9; equal ids: d = 0, a match
                    s_match[a] = 1;
                    s_match[SQ_N + b] = 1;
                }
            }
        }
        __syncthreads();
        if (wave != 0) continue;                                     // no barrier below in this iteration
        // ---- 3. counts and the table, wave 0
        const int qm = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < n1 && s_match[lane] != 0));
        const int cm = __builtin_popcountll(__builtin_amdgcn_ballot_w64(lane < n2 && s_match[SQ_N + lane] != 0));
        double dist = (double)(n1 + n2);                             // one list empty: T[n1][0] or T[0][n2]
        if (n1 > 0 && n2 > 0) {
            const int r = lane + 1;                                  // this lane's row of T
            double prev1 = 0.0, prev2 = 0.0;                         // the row's value on the last two anti-diagonals
            for (int s = 1; s <= n1 + n2; ++s) {
                const int j = s - r;
                double up = __shfl_up(prev1, 1), dg = __shfl_up(prev2, 1);
                if (r == 1) {
                    up = (double)j;                                  // T[0][j]
                    dg = (double)(j - 1);
                }
                double cur = (double)r;                              // j == 0: T[r][0]
                if (r <= n1 && j >= 1 && j <= n2) {
#pragma clang fp contract(off)
                    const double x = up + 1.0, y = prev1 + 1.0, z = dg + cost[(r - 1) * n2 + (j - 1)];
                    cur = x < y ? x : y;
                    cur = z < cur ? z : cur;
                }
                prev2 = prev1;
                prev1 = cur;
            }
            dist = __shfl(prev1, n1 - 1);                            // T[n1][n2], the last cell of row n1
        }
        if (lane == 0) {
#pragma clang fp contract(off)
            const double tot = (double)(n1 + n2);
            ratio[p] = n1 + n2 == 0 ? 1.0 : (tot - dist) / tot;
            qmatch[p] = qm;
            cmatch[p] = cm;
            clen[p] = n2;
        }
    }
}

__global__ __launch_bounds__(64) void k_seq_query_metric(const int* __restrict__ qmatch, const int* __restrict__ cmatch,
                                                         const int* __restrict__ clen, const int* __restrict__ qlen, long nq, int K,
                                                         double* __restrict__ out) {
    const long i = (long)blockIdx.x * 64 + threadIdx.x;
    if (i >= nq) return;
    const int ql = qlen[i];
    double score = 0.0, recall = 0.0;
    for (int j = 0; j < K; ++j) {                                    // ascending j: the canonical order
        const size_t g = (size_t)i * K + j;
        const int cl = clen[g];
        if (cl < 0) continue;
        const int qm = qmatch[g];
        if (ql + cl != 0) score += __ddiv_rn((double)(qm + cmatch[g]), (double)(ql + cl));
        if (ql > 0) recall += __ddiv_rn((double)qm, (double)ql);
    }
    out[i * 2 + 0] = score;
    out[i * 2 + 1] = recall;
}

// ------------------------------------------------------------------------------ host launchers
extern "C" int sss_seq_pair_scores(const int64_t* str_ptr, const int32_t* str_chars, int64_t n_strings, const int64_t* q_ptr,
                                   const int32_t* q_ids, int64_t nq, const int64_t* c_ptr, const int32_t* c_ids, int64_t n,
                                   const int64_t* I, int K, int64_t id_offset, double* ratio, int32_t* qmatch, int32_t* cmatch,
                                   int32_t* clen, int32_t* err, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n_strings <= 0 || n_strings >= (1L << 31) || nq <= 0 || nq >= (1L << 31) || K <= 0 || K > SQ_MAX_K || nq * K >= (1L << 31) ||
        n <= 0 || n >= (1L << 31)) {
        set_error("seq_pair_scores: need 0 < n_strings < 2^31, 0 < nq, nq * K < 2^31, 0 < K <= 1024, 0 < n < 2^31");
        return SSS_EINVAL;
    }
    if (!str_ptr || !str_chars || !q_ptr || !q_ids || !c_ptr || !c_ids || !I || !ratio || !qmatch || !cmatch || !clen || !err) {
        set_error("seq_pair_scores: a null pointer (the string table, both sequence sets, I, the four outputs and err are required)");
        return SSS_EINVAL;
    }
    if (hipMemsetAsync(err, 0, sizeof(int), st) != hipSuccess) { set_error("seq_pair_scores: memset failed"); return SSS_EHIP; }
    const long total = nq * K;
    const unsigned nb = total < (long)SQ_MAX_BLOCKS ? (unsigned)total : SQ_MAX_BLOCKS;
    hipLaunchKernelGGL(k_seq_pair_scores, dim3(nb), dim3(SQ_WAVES * 64), 0, st, str_ptr, str_chars, n_strings, q_ptr, q_ids, nq, c_ptr,
                       c_ids, n, I, K, id_offset, ratio, qmatch, cmatch, clen, err);
    return check_launch("k_seq_pair_scores");
}

extern "C" int sss_seq_query_metric(const int32_t* qmatch, const int32_t* cmatch, const int32_t* clen, const int32_t* qlen, int64_t nq,
                                    int K, double* out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || nq >= (1L << 31) || K <= 0 || K > SQ_MAX_K) {
        set_error("seq_query_metric: need 0 < nq < 2^31, 0 < K <= 1024");
        return SSS_EINVAL;
    }
    if (!qmatch || !cmatch || !clen || !qlen || !out) {
        set_error("seq_query_metric: a null pointer (qmatch, cmatch, clen, qlen and out are required)");
        return SSS_EINVAL;
    }
    const unsigned nb = (unsigned)((nq + 63) / 64);
    hipLaunchKernelGGL(k_seq_query_metric, dim3(nb), dim3(64), 0, st, qmatch, cmatch, clen, qlen, nq, K, out);
    return check_launch("k_seq_query_metric");
}

}  // namespace sss
