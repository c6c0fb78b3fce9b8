// Internal: what a whole workgroup of NT threads (a multiple of 64) does to select and to compact -- the radix descent to
// the k-th largest ordinal, the bitonic sort of u64 keys, a thread's rank among the flagged threads, a workgroup sum.
// Used by the select kernels (select_dev.h), the top-k of a score matrix (topk_scores.hip), the slab compaction
// (slab_compact.h) and hamming.hip's k_hamming_select.  Every function is called by ALL threads of the workgroup under
// uniform control flow, tid = threadIdx.x; the shared words it needs are the caller's.
#pragma once
#include "sss_common.h"

namespace sss {

constexpr int RADIX_HIST_WORDS = 260;   // the descent's shared words: 256 bins, then the picked bin [256] and the rank left in it [257]

// The bin holding the need-th key from the top of a 256-bin histogram s_hist (1 <= need <= the histogram's sum), by ONE
// wave (lane 0 .. 63): four bins a lane, suffix sum by shuffles.  Leaves the bin in s_hist[256] and the rank still to
// find inside it in s_hist[257]; the caller's barrier publishes them.
__device__ __forceinline__ void radix_pick_bin(unsigned* s_hist, unsigned need, int lane) {
    const unsigned h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
    const unsigned mine = h0 + h1 + h2 + h3;
    unsigned suf = mine;                        // sum over this lane and every higher one
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = (unsigned)__shfl_down((int)suf, o);
        if (lane + o < 64) suf += v;
    }
    const unsigned above = suf - mine;
    if (above < need && suf >= need) {          // the need-th from the top falls into this lane's four bins (exactly one lane)
        unsigned cum = above;
        int b = 3;
        if (cum + h3 < need) { cum += h3; b = 2; if (cum + h2 < need) { cum += h2; b = 1; if (cum + h1 < need) { cum += h1; b = 0; } } }
        s_hist[256] = (unsigned)(4 * lane + b);
        s_hist[257] = need - cum;
    }
}

// The k-th largest ordinal among ord_at(0 .. M), 1 <= k <= M: a radix descent, eight bits a pass -- a 256-bin histogram
// (LDS atomics) of the ordinals that still match the prefix, then radix_pick_bin -- four passes over the ordinals instead
// of a sort of them (round 3; it was 32 one-bit passes, 3 barriers each).  What ord_at reads must be visible before the
// call's first barrier.  s_hist: RADIX_HIST_WORDS shared words; every thread returns the same value.
template <int NT, typename OrdAt>
__device__ __forceinline__ unsigned kth_largest_of(OrdAt ord_at, int M, int k, int tid, unsigned* s_hist) {
    unsigned prefix = 0u, mask = 0u;
    unsigned kk = (unsigned)k;                      // rank, from the top, inside the bucket that matches the prefix
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (NT == 256 || tid < 256) s_hist[tid] = 0u;
        __syncthreads();
        for (int x = tid; x < M; x += NT) {
            const unsigned o = ord_at(x);
            if ((o & mask) == prefix) atomicAdd(&s_hist[(o >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) radix_pick_bin(s_hist, kk, tid);
        __syncthreads();
        prefix |= s_hist[256] << shift;
        mask |= 255u << shift;
        kk = s_hist[257];
        __syncthreads();                            // (the two words are rewritten in the next pass)
    }
    return prefix;
}

// Bitonic sort of keys[0 .. M2) in LDS (M2 a power of two), descending (DESC) or ascending; ends on a barrier.
template <int NT, bool DESC>
__device__ __forceinline__ void sort_keys(unsigned long long* keys, int M2, int tid) {
    for (int kk = 2; kk <= M2; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int x = tid; x < M2; x += NT) {
                const int ixj = x ^ j;
                if (ixj > x) {
                    const unsigned long long a = keys[x], b = keys[ixj];
                    const bool desc = ((x & kk) == 0) == DESC;
                    if (desc ? a < b : a > b) { keys[x] = b; keys[ixj] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// RANK IN THREAD ORDER.  Every thread brings F flags; use(before, total) gets, for each flag a, before[a] = the threads
// below this one whose flag a is set and total[a] = all of them (the same in every thread, so a running base lives in
// registers, not in LDS).  Ballot, per-wave popcount to s_wave (F * NT / 64 shared words), barrier, the earlier waves'
// sum (lane w reads wave w's count, a prefix sum inside one DPP row) plus the lanes below, use, barrier.  ONE barrier
// pair whatever F is; use runs between the two, so what it stores retires under the second, which lets the next call
// rewrite s_wave.
template <int NT, int F, typename Use>
__device__ __forceinline__ void block_rank(const bool (&flag)[F], unsigned* s_wave, int tid, Use use) {
    constexpr int NW = NT / 64;
    static_assert(NW <= 16, "the waves' counts are scanned inside one 16-lane DPP row");
    const int lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    unsigned long long b[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
        b[a] = __builtin_amdgcn_ballot_w64(flag[a]);
        if (lane == 0) s_wave[a * NW + wv] = (unsigned)__builtin_popcountll(b[a]);
    }
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned before[F], total[F];
#pragma unroll
    for (int a = 0; a < F; ++a) {
        // lane w < NW holds wave w's count; inclusive prefix over the row (row_shr; lanes without a source add 0)
        const unsigned c = lane < NW ? s_wave[a * NW + lane] : 0u;
        unsigned inc = c;
        inc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)inc, 0x111, 0xf, 0xf, true);
        if (NW > 2) inc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)inc, 0x112, 0xf, 0xf, true);
        if (NW > 4) inc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)inc, 0x114, 0xf, 0xf, true);
        if (NW > 8) inc += (unsigned)__builtin_amdgcn_update_dpp(0, (int)inc, 0x118, 0xf, 0xf, true);
        before[a] = (unsigned)__builtin_amdgcn_readlane((int)(inc - c), wv) + (unsigned)__builtin_popcountll(b[a] & below);
        total[a] = (unsigned)__builtin_amdgcn_readlane((int)inc, NW - 1);
    }
    use(before, total);
    __syncthreads();
}

// Sum over the workgroup of F counters per thread, left in v[] of EVERY thread: shuffle sum, one word per wave, one
// barrier.  s_wave (F * NT / 64 shared words) must not be rewritten while a thread may still read it: once per kernel.
template <int NT, int F>
__device__ __forceinline__ void block_sum(unsigned (&v)[F], unsigned* s_wave, int tid) {
    constexpr int NW = NT / 64;
#pragma unroll
    for (int a = 0; a < F; ++a) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[a] += __shfl_xor(v[a], o);
        if ((tid & 63) == 0) s_wave[a * NW + (tid >> 6)] = v[a];
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < F; ++a) {
        v[a] = 0;
        for (int w = 0; w < NW; ++w) v[a] += s_wave[a * NW + w];
    }
}

}  // namespace sss
