// Internal: one wave per session, one lane per item action -- what the builders of CSR rows share (k_svec_count / _fill in
// sparse.hip: a lane carries its action's item id; k_tbag_count / _fill in ptype.hip: its type through item_type).
//
//   session_compact   the session's item actions compacted onto the lanes in 64-action steps (searches skipped), each as
//                     the value its kernel gives it; the flags word of a session that cannot be a row
//   session_rank      "seen before" by readlane broadcasts over the actions, with the kernel's own accumulation over equal
//                     values; the first occurrences ranked through a ballot
//
// graphbuild.hip's lane_state is another algorithm: its lanes are raw actions and nothing is compacted.
#pragma once
#include "sss_common.h"

namespace sss {

constexpr int SL_MAX_ITEMS = 64;      // item actions per session (one lane each)

// The session of this wave in a launch of 256 threads a workgroup; a wave at or beyond the session count leaves whole.
__device__ __forceinline__ long session_of_wave() { return ((long)blockIdx.x * 256 + threadIdx.x) >> 6; }

struct SessionLane {
    int t;             // the lane
    int L = 0;         // item actions of the session (0 for a flagged session)
    int value = -1;    // the lane's action, as the kernel's value (-1: no action, or one that counts for nothing)
    bool first;        // this lane holds the first occurrence of its value
    int rank;          // ... and its position among the distinct values, ascending
    int m;             // distinct values of the session
};

// Lane t of the wave <- the t-th item action of the wave's session, as value_of(item id, bad): an int >= 0, or -1 for an
// action that counts for nothing; value_of may raise bit 1 or bit 2 of `bad` for an id it cannot take.  err bit 0: more than
// 64 item actions (or a decreasing sess_ptr); bits 1 and 2: the OR of `bad` over the session.  A flagged session counts as
// empty, in a count and in a fill alike, so every write stays inside the session's own range.  s = session_of_wave(), below
// the session count.
template <class ValueOf>
__device__ __forceinline__ SessionLane session_compact(const long* __restrict__ sess_ptr, const unsigned char* __restrict__ is_search,
                                                       const long* __restrict__ item_id, long s, int* __restrict__ err,
                                                       ValueOf value_of) {
    __shared__ int slots[4 * SL_MAX_ITEMS];
    SessionLane Ln;
    const int t = Ln.t = threadIdx.x & 63;
    volatile int* slot = slots + (threadIdx.x >> 6) * SL_MAX_ITEMS;
    const long a0 = sess_ptr[s], a1 = sess_ptr[s + 1];
    const unsigned long long lt = t == 0 ? 0ull : (~0ull >> (64 - t));
    int L = 0, bad = 0;
    for (long base = a0; base < a1; base += 64) {                // wave-uniform trip count
        const long a = base + t;
        const bool clk = a < a1 && is_search[a] == 0;
        const long it = clk ? item_id[a] : 0;
        const unsigned long long cm = __builtin_amdgcn_ballot_w64(clk);
        const int dest = L + __builtin_popcountll(cm & lt);
        if (clk) {
            const int v = value_of(it, bad);
            if (dest < SL_MAX_ITEMS) slot[dest] = v;
        }
        L += __builtin_popcountll(cm);
    }
    __builtin_amdgcn_wave_barrier();
    int flags = (L > SL_MAX_ITEMS || a1 < a0) ? 1 : 0;
    for (int bit = 2; bit <= 4; bit <<= 1)
        if (__builtin_amdgcn_ballot_w64((bad & bit) != 0) != 0ull) flags |= bit;
    if (flags) {
        if (t == 0) atomicOr(err, flags);
        L = 0;
    }
    Ln.L = L;
    Ln.value = t < L ? slot[t] : -1;
    __builtin_amdgcn_wave_barrier();
    return Ln;
}

// first / rank / m of a compacted session.  each(u, hit) runs for every item action u of the session, wave-uniformly (it
// may broadcast from lane u): `hit` on the lanes whose value is action u's, so the kernel accumulates over equal values.
template <class Each>
__device__ __forceinline__ void session_rank(SessionLane& Ln, Each each) {
    const bool live = Ln.value >= 0;
    bool seen = false;
    for (int u = 0; u < Ln.L; ++u) {                             // uniform loop: broadcast item action u
        const int vu = __builtin_amdgcn_readlane(Ln.value, u);  // by every lane: behind `live &&` it would be a branch
        const bool hit = live && vu == Ln.value;
        if (hit && u < Ln.t) seen = true;
        each(u, hit);
    }
    Ln.first = live && !seen;
    const unsigned long long fm = __builtin_amdgcn_ballot_w64(Ln.first);
    Ln.m = __builtin_popcountll(fm);
    Ln.rank = 0;
    for (unsigned long long todo = fm; todo; todo &= todo - 1) {
        const int vu = __builtin_amdgcn_readlane(Ln.value, __builtin_ctzll(todo));
        if (Ln.first && vu < Ln.value) ++Ln.rank;
    }
}

// ------------------------------------------------------------------------------ host
// The arguments every builder entry point takes, checked (the ranges, then the pointers; messages start with `what`), and
// *nb: the workgroups of its launch, 256 threads each, one wave a session.
static int session_args(const char* what, const void* sess_ptr, const void* is_search, const void* item_id, long S, long n_items,
                        const void* err, unsigned* nb) {
    if (S <= 0 || S >= (1L << 31) || n_items <= 0 || n_items > 0x7fffffffL) {
        set_error("%s: need 0 < n_sessions < 2^31, 0 < n_items < 2^31", what);
        return SSS_EINVAL;
    }
    if (!sess_ptr || !is_search || !item_id || !err) {
        set_error("%s: a null pointer (sess_ptr, is_search, item_id and err are required)", what);
        return SSS_EINVAL;
    }
    *nb = (unsigned)((S * 64 + 255) / 256);
    return SSS_OK;
}

}  // namespace sss
