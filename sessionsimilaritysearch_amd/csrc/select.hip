// The fused search's select: candidate selection + canonical float64 re-score + proof of exactness
// (gfx950).  Second half of what the reference asks of faiss at
// test_amazon_filterd.py:578 (the per-query heap inside IndexFlatIP.search).
//
// Input: the compact candidate keys k_scan (scan.hip) appended per query.  Per query:
//   select the best K2 = k + slack candidates by (scan score desc, id asc), re-score them in
//   float64 from the stored rows in the canonical sequential order (== the oracle's score), order by
//   (score desc, id asc), write the first k, and decide
//   status[q] = 0  proven exact: every row that was NOT re-scored has a scan score at or below
//                  the selection edge (it lost to a full list's tail <= edge, or to the admission
//                  threshold < edge, or it is a candidate ranked below the edge), and
//                  edge + B + one float32 ulp < k-th re-scored score, B bounding the error of the
//                  scan that produced the candidates (select_dev.h: err_bound; DT_F16 scores are first divided by
//                  the query's and the corpus' power-of-two scales);
//            != 0  not proven (bit 0: a full list's tail outranks the edge, bit 1: the admission
//                  threshold does, bit 2: near-tie window) -> the caller re-runs the query through
//                  the threshold rung (select_thr.hip) or the exhaustive path.
//   k_select_fast  : one wave per query, K2 <= 16, candidates <= FS_CAP (the common case: the
//                    shared threshold leaves a few hundred candidates per query); a query that fails
//                    ONLY the near-tie window gets a second chance with up to 32 candidates
//   k_select_sort  : one workgroup per query, bitonic sort in LDS, any K2 <= SEL_MAX_K2
#include "select_dev.h"

namespace sss {

constexpr int FS_CAP = 2048;       // candidates a wave stages in LDS (more -> unproven)
constexpr int FS_K2 = 32;          // candidates the wave-per-query kernel can re-score (its second chance widens K2 <= 16 up to this)
constexpr int FS_COL = 16;         // candidate keys a lane keeps in registers (64 x 16 = 1024 candidates; more -> columns in LDS)
constexpr int SEL_MAX_K2 = 512;

// Hand the query's state words back zeroed (scan.h: the contract that replaces a per-call memset).
__device__ __forceinline__ void clear_state(const SelectArgs& A, int q, int t, int nthreads) {
    for (int j = t; j < A.J; j += nthreads) A.slots[(size_t)q * SLOT_STRIDE + j] = 0u;
    if (t == 0) { A.cnt[q] = 0u; A.maxlast[q] = 0ull; }
}

// The scan's final threshold word of query q from its J slots (0: not enough classes ever published): the min, or --
// rank-selected scans (cert == 1, J == 16: scan_dev.h tau_select16) -- the exact (skip + 1)-th smallest of the 16
// (the scan's own, cheaper pick lies at or below it).
// Called by a whole wave.
__device__ __forceinline__ unsigned final_tau_ord(const unsigned* slots, int J, int lane, int skip) {
    if (skip > 0 && J == 16) {
        const unsigned mine = slots[lane & 15];
        int rank = 0;                                             // values ordered by (word, slot index): ranks 0 .. 15
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const unsigned o = (unsigned)__shfl((int)mine, j);
            rank += (o < mine || (o == mine && j < (lane & 15))) ? 1 : 0;
        }
        const unsigned long long own = __builtin_amdgcn_ballot_w64(lane < 16 && rank == skip);
        return (unsigned)__builtin_amdgcn_readlane((int)mine, __builtin_ctzll(own));
    }
    unsigned m = 0xFFFFFFFFu;
    for (int j = lane; j < J; j += 64) m = min(m, slots[j]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, (unsigned)__shfl_xor((int)m, o));
    return m;
}

// Shared tail: rank the K2 re-scored candidates, write results, decide the status.  Called by
// the threads [0, nthreads) of one query with sel/resc in LDS; lane0 writes the status.
template <int NT>
__device__ __forceinline__ void rank_and_write(const unsigned long long* sel, const double* resc, int K2, int k,
                                               long id_offset, float* Dq, long* Iq, int t, int* s_nvalid,
                                               double* s_kth, int metric) {
    for (int c = t; c < K2; c += NT) {
        const unsigned long long key = sel[c];
        const int id = key_id(key);
        if (key == 0 || id < 0) continue;
        const float sc = (float)resc[c];
        int rank = 0;
        for (int j = 0; j < K2; ++j) {
            const int idj = key_id(sel[j]);
            if (j == c || sel[j] == 0 || idj < 0) continue;
            const float sj = (float)resc[j];
            if (sj > sc || (sj == sc && idj < id)) ++rank;
        }
        atomicAdd(s_nvalid, 1);
        if (rank < k) { Dq[rank] = out_score(sc, metric); Iq[rank] = (long)id + id_offset; }
        if (rank == k - 1) *s_kth = resc[c];
    }
}

// A row outside the candidates has scan score <= the edge's, so its exact score is <= edge * unscale + B; it can
// neither enter the top k nor tie with the k-th result AFTER the rounding to float32 if that stays
// below kth by more than one float32 ulp of kth (select_dev.h: window_top).
__device__ __forceinline__ int decide_status(unsigned long long edge, unsigned long long maxlast, unsigned tau_o,
                                             int J, int nvalid, int k, double kth, double B, double unscale, double off) {
    int st = 0;
    const bool edge_real = edge != 0 && key_id(edge) >= 0;
    if (maxlast > edge) st |= 1;                                  // a full list may hide a contender
    if (J > 0 && tau_o > ORD_NEG_INF) {                           // rows were rejected at or below ord2f(tau_o - 1)
        if (!(edge_real && f2ord(key_score(edge)) >= tau_o)) st |= 2;
    }
    if (edge_real && nvalid >= k) {
        if (!(window_top(key_score(edge), unscale, off, B, kth) < kth)) st |= 4;                              // the error window reaches the k-th result
    }
    return st;
}

// ------------------------------------------------------------------------------------------
// One wave per query.  LDS per wave: keys[FS_CAP] | sel[FS_K2] | resc[FS_K2] | counters | qrow[rb]
__global__ __launch_bounds__(256) void k_select_fast(const SelectArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + wv;
    if (q >= A.nq) return;                                        // whole wave; no block-level sync below
    const int rb = row_bytes(A.d, A.dtype), rbc = stored_row_bytes(A);      // a query row, a stored row
    const size_t per_wave = (size_t)FS_CAP * 8 + FS_K2 * 16 + 16 + rb;
    char* base = smem + wv * ((per_wave + 15) & ~(size_t)15);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(base);
    unsigned long long* sel = keys + FS_CAP;
    double* resc = reinterpret_cast<double*>(sel + FS_K2);
    int* s_nvalid = reinterpret_cast<int*>(resc + FS_K2);
    double* s_kth = reinterpret_cast<double*>(s_nvalid + 2);
    char* qrow = reinterpret_cast<char*>(s_kth + 1);

    const int K2 = A.K2, k = A.k;
    float* Dq = A.D_out + (size_t)q * k;
    long* Iq = A.I_out + (size_t)q * k;
    const int M = (int)min(A.cnt[q], (unsigned)A.cap);            // (the append form of k_scan counts what it could not store, too)
    if (M > FS_CAP) {                                             // adversarial input: let the exhaustive path decide
        pad_results(Dq, Iq, 0, k, lane, 64, A.metric);            // (no k-th score known)
        if (lane == 0) { A.status[q] = 1; if (A.unproven_count) atomicAdd(A.unproven_count, 1); }
        clear_state(A, q, lane, 64);
        return;
    }
    // ---- the query row, and this lane's COLUMN of the candidate keys (keys lane, lane + 64, ...).  Up to 1024
    // candidates (the usual few hundred) a column is 16 keys in registers, sorted once by a bitonic network: a
    // selection round is then one wave-wide maximum of the column heads and a register shift in the owner lane.
    // More candidates: columns stay in LDS and the owner rescans its column after every round (as in round 2,
    // when this was the only form and the 16 rounds took 40 % of the kernel).
    const unsigned long long* ck = A.cand + (size_t)q * A.cap;
    const bool in_regs = M <= 64 * FS_COL;                        // wave-uniform
    unsigned long long col[FS_COL];
    unsigned long long best = 0; int bidx = -1;
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < FS_COL; ++j) col[j] = lane + 64 * j < M ? ck[lane + 64 * j] : 0ull;
#pragma unroll
        for (int kk = 2; kk <= FS_COL; kk <<= 1)
#pragma unroll
            for (int jj = kk >> 1; jj > 0; jj >>= 1)
#pragma unroll
                for (int x = 0; x < FS_COL; ++x) {
                    const int y = x ^ jj;
                    if (y > x) {
                        const unsigned long long a = col[x], b = col[y];
                        const bool sw = ((x & kk) == 0) ? a < b : a > b;      // descending overall
                        col[x] = sw ? b : a; col[y] = sw ? a : b;
                    }
                }
        best = col[0];
    } else {
        for (int i = lane; i < M; i += 64) {
            const unsigned long long v = ck[i];
            keys[i] = v;
            if (v > best) { best = v; bidx = i; }
        }
    }
    // the owner of the round's maximum retires it: its next-best key becomes its column head
    auto retire = [&]() __attribute__((always_inline)) {
        if (in_regs) {
#pragma unroll
            for (int j = 0; j + 1 < FS_COL; ++j) col[j] = col[j + 1];
            col[FS_COL - 1] = 0ull;
            best = col[0];
        } else {
            keys[bidx] = 0;
            best = 0; bidx = -1;
            for (int i = lane; i < M; i += 64) {
                const unsigned long long v = keys[i];
                if (v > best) { best = v; bidx = i; }
            }
        }
    };
    load_query_row<64>(qrow, A.Q, q, rb, lane);
    if (lane == 0) { *s_nvalid = 0; *s_kth = 0.0; }
    wave_sync();
    // ---- K2 rounds: wave-wide arg-max, the owner lane retires its key
    for (int it = 0; it < K2; ++it) {
        const unsigned long long w = wave_max_u64(best);
        if (lane == 0) sel[it] = w;
        if (w != 0 && best == w) retire();                        // keys of real candidates are unique
    }
    wave_sync();
    // ---- float64 re-score: one lane per candidate walks its corpus row (16-byte loads straight from
    // L2 / HBM, several in flight) sequentially in k -- the canonical order
    const int rtype = rescore_type(A.dtype, A.metric);
    for (int c0 = 0; c0 < K2; c0 += 16) rescore16(sel, resc, c0, K2, A.C, rbc, qrow, rtype, lane);
    double B, unscale, off;
    query_bound(A, qrow, lane, B, unscale, off);
    wave_sync();
    rank_and_write<64>(sel, resc, K2, k, A.id_offset, Dq, Iq, lane, s_nvalid, s_kth, A.metric);
    wave_sync();
    const int nvalid = *s_nvalid;
    pad_results(Dq, Iq, nvalid, k, lane, 64, A.metric);
    const unsigned tau_o = A.J > 0 ? final_tau_ord(A.slots + (size_t)q * SLOT_STRIDE, A.J, lane, A.tau_skip) : 0u;
    const unsigned long long maxlast = A.maxlast[q];
    wave_sync();                                                  // every lane has read the state words
    clear_state(A, q, lane, 64);
    int st = decide_status(sel[K2 - 1], maxlast, tau_o, A.J, nvalid, k, *s_kth, B, unscale, off);
    // ---- second chance for a query whose ONLY problem is the near-tie window (status 4): the pool
    // usually holds more candidates than the K2 the threshold certifies, and it is complete down to
    // max(threshold, largest tail of a full list).  Take candidates from that region -- until the next one
    // already lies below the k-th result by more than the error window (the k-th result can only rise when
    // candidates are added), up to FS_K2 in all -- re-score the new ones, rank again; what stays outside
    // is bounded by the first key not taken (or by the region's floor).
    if (st == 4 && K2 < FS_K2) {                                  // wave-uniform (all lanes computed st)
        const bool has_tau = A.J > 0 && tau_o > ORD_NEG_INF;
        int K2x = K2;
        float edge_score = -INFINITY;
        bool open_end = false;                                    // stopped by the budget: edge = last key taken
        const double kth0 = *s_kth;                               // lower bound of the final k-th result
        for (; K2x < FS_K2; ++K2x) {
            const unsigned long long w = wave_max_u64(best);
            if (w != 0 && key_id(w) >= 0 && window_top(key_score(w), unscale, off, B, kth0) < kth0) {
                edge_score = key_score(w);                        // far enough below: nothing from here on can matter
                break;
            }
            const bool inside = w != 0 && key_id(w) >= 0 && w >= maxlast && (!has_tau || f2ord(key_score(w)) >= tau_o);
            if (!inside) {
                if (w != 0 && key_id(w) >= 0) edge_score = key_score(w);
                break;
            }
            if (lane == 0) sel[K2x] = w;
            if (best == w) retire();
        }
        if (K2x == FS_K2) open_end = true;
        wave_sync();
        if (K2x > K2) {
            for (int c0 = K2; c0 < K2x; c0 += 16) rescore16(sel, resc, c0, K2x, A.C, rbc, qrow, rtype, lane);
            if (lane == 0) { *s_nvalid = 0; *s_kth = 0.0; }
            wave_sync();
            rank_and_write<64>(sel, resc, K2x, k, A.id_offset, Dq, Iq, lane, s_nvalid, s_kth, A.metric);
            wave_sync();
        }
        // (K2x == K2: the very next candidate already lies far below -- phase 1 only failed because it
        //  measures the window from the last INCLUDED key)
        if (open_end) {
            edge_score = key_score(sel[K2x - 1]);
        } else {                                                  // everything else lies under the region's floor
            if (has_tau) edge_score = fmaxf(edge_score, ord2f(tau_o - 1));
            if (maxlast != 0 && key_id(maxlast) >= 0) edge_score = fmaxf(edge_score, key_score(maxlast));
        }
        const double kth = *s_kth;
        st = (*s_nvalid >= k && window_top(edge_score, unscale, off, B, kth) < kth) ? 0 : 4;
    }
    if (A.metric && !(B < INFINITY)) st |= 4;                     // no finite L2 bound (select_dev.h: err_bound_l2): nothing is proven
    if (lane == 0) {
        A.status[q] = st;
        if (st && A.unproven_count) atomicAdd(A.unproven_count, 1);
    }
}

// ------------------------------------------------------------------------------------------
// One workgroup per query: bitonic sort (descending) of the candidate keys in LDS.
__global__ __launch_bounds__(SORT_THREADS) void k_select_sort(const SelectArgs A, int cap_pow2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);             // [cap_pow2]
    double* resc = reinterpret_cast<double*>(keys + cap_pow2);                           // [SEL_MAX_K2]
    char* qrow = reinterpret_cast<char*>(resc + SEL_MAX_K2);
    __shared__ int s_nvalid;
    __shared__ double s_kth;
    __shared__ unsigned s_hist[260];
    __shared__ unsigned s_cnt;
    const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int rb = row_bytes(A.d, A.dtype), rbc = stored_row_bytes(A);      // a query row, a stored row
    const int K2 = A.K2, k = A.k;
    float* Dq = A.D_out + (size_t)q * k;
    long* Iq = A.I_out + (size_t)q * k;
    const int M = (int)min(A.cnt[q], (unsigned)A.cap);            // (the append form of k_scan counts what it could not store, too)
    int M2 = 64;
    while (M2 < M || M2 < K2) M2 <<= 1;                            // <= cap_pow2 by construction
    const unsigned long long* ck = A.cand + (size_t)q * A.cap;
    for (int i = tid; i < M2; i += SORT_THREADS) keys[i] = i < M ? ck[i] : 0ull;
    load_query_row<SORT_THREADS>(qrow, A.Q, q, rb, tid);
    if (tid == 0) { s_nvalid = 0; s_kth = 0.0; }
    __syncthreads();
    // Only the K2 best candidates are needed, in order: with many more than that (the lists of a k = 500 search hold up to
    // 2048), they are SELECTED first (kth_largest_key) and only they are sorted -- 45 barrier stages over 512 keys instead of
    // 66 over 2048.  (The re-score slots serve as the compaction buffer: nothing has been re-scored yet.)
    int Ms = M2;
    {
        int K2p = 64;
        while (K2p < K2) K2p <<= 1;
        if (M > 2 * K2p) {
            const unsigned long long T = kth_largest_key(keys, M, K2, tid, s_hist, &s_cnt);
            unsigned long long* tmp = reinterpret_cast<unsigned long long*>(resc);
            __syncthreads();
            if (tid == 0) s_cnt = 0u;
            __syncthreads();
            for (int x = tid; x < M; x += SORT_THREADS) {
                const unsigned long long kx = keys[x];
                if (kx >= T) tmp[atomicAdd(&s_cnt, 1u)] = kx;
            }
            __syncthreads();
            for (int x = tid; x < K2p; x += SORT_THREADS) keys[x] = x < K2 ? tmp[x] : 0ull;
            __syncthreads();
            Ms = K2p;
        }
    }
    sort_desc(keys, Ms, tid);
    // ---- float64 re-score straight from global (one thread per candidate, sequential in k)
    for (int c = tid; c < K2; c += SORT_THREADS) {
        const unsigned long long key = keys[c];
        const int id = key_id(key);
        double acc = 0.0;
        if (key != 0 && id >= 0) acc = rescore_row(qrow, reinterpret_cast<const char*>(A.C) + (size_t)id * rbc, rbc / 16, rescore_type(A.dtype, A.metric));
        resc[c] = acc;
    }
    __syncthreads();
    rank_and_write<SORT_THREADS>(keys, resc, K2, k, A.id_offset, Dq, Iq, tid, &s_nvalid, &s_kth, A.metric);
    __syncthreads();
    const int nvalid = s_nvalid;
    pad_results(Dq, Iq, nvalid, k, tid, SORT_THREADS, A.metric);
    if (tid < 64) {                                               // wave 0 alone touches the state from here on
        const unsigned tau_o = A.J > 0 ? final_tau_ord(A.slots + (size_t)q * SLOT_STRIDE, A.J, lane, A.tau_skip) : 0u;
        const unsigned long long maxlast = A.maxlast[q];
        wave_sync();
        clear_state(A, q, lane, 64);
        double B, unscale, off;
        query_bound(A, qrow, lane, B, unscale, off);
        if (tid == 0) {
            int st = decide_status(keys[K2 - 1], maxlast, tau_o, A.J, nvalid, k, s_kth, B, unscale, off);
            if (A.metric && !(B < INFINITY)) st |= 4;             // (as k_select_fast)
            A.status[q] = st;
            if (st && A.unproven_count) atomicAdd(A.unproven_count, 1);
        }
    }
}

// ------------------------------------------------------------------------------ host side
int launch_select(const SelectArgs& a, hipStream_t st) {
    const int rb = a.d * elem_bytes(a.dtype);
    // the wave-per-query kernel serves the K2 <= 16 regime (class maxima + bootstrap: a few hundred
    // candidates per query); beyond it the lists run without the bootstrap and fill up (thousands of
    // candidates, more than a wave stages), which is the sort kernel's job
    if (a.K2 <= KP) {
        const size_t per_wave = (((size_t)FS_CAP * 8 + FS_K2 * 16 + 16 + rb) + 15) & ~(size_t)15;
        const size_t lds = 4 * per_wave;
        const int rc = opt_in_lds(reinterpret_cast<const void*>(&k_select_fast), "k_select_fast", 160 * 1024 - 1024);
        if (rc) return rc;
        hipLaunchKernelGGL(k_select_fast, dim3((unsigned)((a.nq + 3) / 4)), dim3(256), lds, st, a);
        return check_launch("k_select_fast");
    }
    if (a.K2 > SEL_MAX_K2) { set_error("select: K2 %d > %d", a.K2, SEL_MAX_K2); return SSS_EINVAL; }
    const int cap_pow2 = pow2_at_least(a.cap > a.K2 ? a.cap : a.K2);
    const size_t lds = (size_t)cap_pow2 * 8 + SEL_MAX_K2 * 8 + rb;
    if (lds > 150 * 1024) { set_error("select: candidate capacity %d too large", a.cap); return SSS_EINVAL; }
    const int rc = opt_in_lds(reinterpret_cast<const void*>(&k_select_sort), "k_select_sort", 160 * 1024 - 4096);   // (its static words take ~1.1 KB)
    if (rc) return rc;
    hipLaunchKernelGGL(k_select_sort, dim3((unsigned)a.nq), dim3(SORT_THREADS), lds, st, a, cap_pow2);
    return check_launch("k_select_sort");
}

}  // namespace sss
