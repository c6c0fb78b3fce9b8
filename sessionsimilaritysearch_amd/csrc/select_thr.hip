// The threshold form of the search (gfx950): a known lower bound of a query's k-th score -- or the caller's radius --
// becomes a scan threshold (select_dev.h: thr_from_bound), k_scan<..., THR> / the long-row scan keep EVERY row above it,
// and the kept rows are re-scored canonically in float64.  Serves the threshold rung behind the fused search (select.hip),
// sss_ip_topk_long (scan_long.hip) and range search (ip_topk.hip).
#include "select_dev.h"

namespace sss {

constexpr int SA_ROWS_SMALL = 256;                 // k_select_all: survivors re-scored per group (one thread each): the first launch (<= 2048 kept rows) --
                                                   //   k + a few dozen survivors are ONE group up to k = 200-odd (a second group doubles the workgroup's time)
constexpr int SA_ROWS_FULL = 128;                  //   ... the full-capacity launch (128 KB of keys leave room for no more)

// ------------------------------------------------------------------------------------------
// THRESHOLD RUNG (between the fused search and the exhaustive kernels).  A query the fused search left
// unproven still has a valid LOWER BOUND of its k-th best score: lb = its k-th re-scored candidate.  A row
// whose exact score could reach lb (or tie with it after the rounding to float32) has a scan score above
//     thr = (lb - B - one float32 ulp of lb) / unscale          (select_dev.h: the proof window, thr_from_bound)
// so ONE more scan of the corpus for just those queries (k_scan<..., THR>) that keeps EVERY row above thr,
// followed by the canonical re-score of all of them, is exact whatever the reason the proof failed -- near
// ties inside the scan's error window and exact ties (duplicate rows) alike -- as long as the rows above thr
// fit the candidate capacity; otherwise the query stays unproven and goes to the exhaustive kernels.
//
// k_thr_prepare: one wave per selected query: its threshold in the scan's domain, counter zeroed.
// B and unscale of selected query i = row q (select_dev.h: query_bound; ONE wave), through the `qb` cache when there is one.
// (the cache of the long-row searches: [nsel] (B, unscale) pairs -- off = 0 for the inner product -- and, metric 1, the [nsel]
//  off = -|q|^2 and the [nsel] bounds of k_select_all's pruning behind them; there B is the per-query REST of the per-row bound)
__device__ __forceinline__ void query_bound(const ThrArgs& A, int i, int q, int lane, double& B, double& unscale, double& off) {
    if (A.qb != nullptr && A.qb_ready) {                                    // (selected query i = row q)
        B = A.qb[2 * (size_t)i]; unscale = A.qb[2 * (size_t)i + 1];
        off = A.metric ? A.qb[2 * (size_t)A.nsel + i] : 0.0;
        return;
    }
    query_bound(A, reinterpret_cast<const char*>(A.Q) + (size_t)q * row_bytes(A.d, A.dtype), lane, B, unscale, off);
    if (A.qb != nullptr && lane == 0) {
        A.qb[2 * (size_t)i] = B; A.qb[2 * (size_t)i + 1] = unscale;
        if (A.metric) A.qb[2 * (size_t)A.nsel + i] = off;
    }
}

// L2 on long rows: a query whose bound is not finite (sigma or a scaled bias beyond float32's range, select_dev.h:
// err_bound_l2) has scan keys that prove nothing -- a scaled bias that overflowed is -inf, which no threshold keeps.  Its
// threshold is +inf at every level: it keeps no row, stays at status 1 and is resolved by the exhaustive kernels.
__device__ __forceinline__ float long_thr(const ThrArgs& A, float thr, double B) {
    return A.metric && !(B < (double)INFINITY) ? INFINITY : thr;
}

// THE PER-ROW BOUND (L2 on long rows).  err_bound_l2 bounds |key -> score - exact score| of EVERY row through the largest
// corpus norm cmax.  On a corpus whose norms are spread, the rows nearest to a query are the small ones, whose own error
// is far smaller -- and a proof window 2 B_l2(cmax) wide holds tens of thousands of them at 1M rows.  Every term of
// err_bound_l2 holds row by row with |c| in place of cmax (cmax only ever stands for "at least |c|"), and the row's f16
// residual norm is at most 2^-11 |c| + rho0 (an element that lands in the f16 normal range is rounded to 11 significant
// bits; one below it -- 2^-14 in the scaled domain -- moves by at most 2^-25 there: rho0 = sqrt(d) 2^-25 / 2^corpus_shift).
// With qn = |q|, rq = the query's residual norm, g = 2^-25 sqrt(d + 1) + (d + 1) 2^-23, A = (d + 4) 2^-23 (three roundings
// more than err_bound_l2 counts: the seed is a sum of two rounded products now, not an exact one), the bound of a row is
//     err(c) = P |c| + Q |c|^2 + R,
//     P = 2.04 (2^-11 qn + (1 + 2^-11) rq + g qn) + 1.02 (d + 3) 2^-52 2 qn
//     Q = 2.04 A / 2 + 1.02 (2^-24 + (d + 3) 2^-52)
//     R = 2.04 (rho0 (qn + rq) + 2^-126 / sigma) + 1.02 (2^-149 + (3 d + 8) 2^-53 qn^2) + P 2^-74
// (the last term: a bias in the float32 subnormal range gives the scan a norm that may be 2^-74 short).  In the scan's
// domain (score = key 2 / sigma + off) that is sigma / 2 err(c), and -2 bias is |c|^2: the scan LOWERS a key by it with the
// seed sigma (1 + Q) bias - sigma P / 2 |c| and RAISES it with sigma (1 - Q) bias + sigma P / 2 |c| (P and Q inflated by
// 1e-3 for the float32 roundings of the coefficients and of the norm the scan derives from the bias).  Then
//   * a LOWERED key maps to a score at most R above the exact one: the k-th largest lowered key of a sample is a lower
//     bound of the k-th score with B = R (k_bound_prepare as it is);
//   * a RAISED key maps to a score at least the exact one minus R: on the last level a row that is not kept (raised key
//     <= thr_from_bound(lb, R, ...)) cannot reach lb -- the proof k_select_all needs, with a window of the NEAR rows' own
//     errors.  Sample levels compare lowered keys with that threshold: they keep fewer rows, which a lower bound allows;
//   * k_select_all prunes the kept rows of the last level by raised keys, which lie within 2 err(cmax) + R of the exact
//     score: its B is 3 max(B_l2(cmax), err(cmax)), the fourth array of the cache.
// Writes the four seed coefficients of query i ([2][2][nsel]: lowered (k0, k1), raised (k0, k1)) and the cache entries;
// ONE wave.  B_glob: err_bound_l2 of the query (infinite: zeros -- the query keeps nothing).
__device__ __forceinline__ void l2_long_bound(const ThrArgs& A, int i, int lane, double B_glob, double unscale, float* __restrict__ seed) {
    const float* row = reinterpret_cast<const float*>(A.Q) + (size_t)i * A.d;
    double qn2 = 0.0;
    float amax = 0.f;
    for (int kk = lane; kk < A.d; kk += 64) { const float v = row[kk]; qn2 += (double)v * (double)v; amax = fmaxf(amax, fabsf(v)); }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { qn2 += __shfl_xor(qn2, o); amax = fmaxf(amax, __shfl_xor(amax, o)); }
    const int sh = f16_shift(amax);
    double rq2 = 0.0;
    for (int kk = lane; kk < A.d; kk += 64) rq2 += f16_resid2(row[kk], sh);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) rq2 += __shfl_xor(rq2, o);
    if (lane != 0) return;
    const double d = (double)A.d, qn = sqrt(qn2), rq = sqrt(rq2), cmax = (double)A.corpus_max_norm;
    const double sigma = 2.0 / unscale;                                     // (unscale: the L2 one, 2 / sigma)
    const double rho0 = sqrt(d) * 2.98023223876953125e-08 * ldexp(1.0, -A.corpus_shift);
    const double g = 2.98023223876953125e-08 * sqrt(d + 1.0) + (d + 1.0) * 1.1920928955078125e-07;
    const double Aq = (d + 4.0) * 1.1920928955078125e-07;
    const double P = 2.04 * (4.8828125e-04 * qn + (1.0 + 4.8828125e-04) * rq + g * qn) + 1.02 * (d + 3.0) * 2.220446049250313e-16 * 2.0 * qn;
    const double Q = 2.04 * Aq * 0.5 + 1.02 * (5.9604644775390625e-08 + (d + 3.0) * 2.220446049250313e-16);
    const double R = 2.04 * (rho0 * (qn + rq) + 1.1754943508222875e-38 / sigma) +
                     1.02 * (1.4012984643248171e-45 + (3.0 * d + 8.0) * 1.1102230246251565e-16 * qn2) + P * 5.293955920339377e-23;
    const double errmax = P * cmax + Q * cmax * cmax + R;
    const bool ok = B_glob < (double)INFINITY && errmax == errmax && errmax < 1.0e300;
    const double Pi = P * 1.001, Qi = Q * 1.001;
    const size_t ns = (size_t)A.nsel;
    seed[i] = ok ? (float)(sigma * (1.0 + Qi)) : 0.f;
    seed[ns + i] = ok ? (float)(-0.5 * sigma * Pi) : 0.f;
    seed[2 * ns + i] = ok ? (float)(sigma * (1.0 - Qi)) : 0.f;
    seed[3 * ns + i] = ok ? (float)(0.5 * sigma * Pi) : 0.f;
    A.qb[2 * (size_t)i] = ok ? R : (double)INFINITY;
    A.qb[3 * ns + i] = ok ? 3.0 * fmax(B_glob, errmax) : (double)INFINITY;
}

// the bound k_select_all prunes with: the query's B, or -- long-row L2, whose cached B is the rest R -- the cache's fourth array
__device__ __forceinline__ double select_bound(const ThrArgs& A, int i, double B) {
    return A.metric && A.qb != nullptr && A.qb_ready ? A.qb[3 * (size_t)A.nsel + i] : B;
}

// keep mode (one wave): the rows kept so far were kept under an OLDER, lower threshold over tiles the next scan will not
// visit again; those that pass the new one stay (compacted in place, in order: a lane writes at or below the index it
// read, and the whole wave has read a chunk before any of it is written).  An overflowed array stays overflowed.
__device__ __forceinline__ void prune_kept(const ThrArgs& A, int i, float thr, int lane) {
    const unsigned M = A.cnt[i];
    if (M > (unsigned)A.cap) return;
    unsigned long long* ck = const_cast<unsigned long long*>(A.cand) + (size_t)i * A.cap;
    unsigned out = 0u;
    for (unsigned c0 = 0; c0 < M; c0 += 64) {
        const unsigned c = c0 + lane;
        const unsigned long long key = c < M ? ck[c] : 0ull;
        const bool kp = c < M && key_score(key) > thr;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(kp);
        const unsigned pos = out + (unsigned)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
        if (kp) ck[pos] = key;
        out += (unsigned)__builtin_popcountll(mask);
    }
    if (lane == 0) A.cnt[i] = out;
}

__global__ __launch_bounds__(256) void k_thr_prepare(const ThrArgs A) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.nsel) return;
    const int q = A.qsel[i];
    double B, unscale, off;
    query_bound(A, i, q, lane, B, unscale, off);                            // (every lane ends up with the same B / unscale)
    // (L2: the k-th distance already known is an UPPER bound of the true one: negated, a lower bound of the k-th score)
    const float thr = thr_from_bound((double)out_score(A.D_out[(size_t)q * A.k + A.k - 1], A.metric), B, unscale, off);    // -FLT_MAX when no k-th score is known
    if (lane == 0) A.thr[i] = thr;
    if (!A.keep) {
        if (lane == 0) A.cnt[i] = 0u;
        return;
    }
    prune_kept(A, i, thr, lane);
}

// sss_ip_topk_long / sss_l2_topk_long, before the first scan: one wave per query (scan.h: launch_long_setup).
// D_out's rows start at "no bound known" in the domain the caller reads -- -FLT_MAX scores, +FLT_MAX distances (metric 1) --
// and column k-1 stays in that domain while the levels run: k_bound_prepare converts on the way in and out (out_score).
// seed (L2): the scan's seed coefficients per query (THE PER-ROW BOUND above), from sigma = 2^(corpus_shift + the query's
// shift) -- the shift query_bound re-derives; zeros where the query's bound is infinite (it keeps nothing: no inf or NaN
// enters the seeding MFMA).
__global__ __launch_bounds__(256) void k_long_setup(const ThrArgs A, int* __restrict__ qsel, _Float16* __restrict__ qimg,
                                                    float* __restrict__ seed) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.nsel) return;
    if (qimg != nullptr) {                          // f32 queries -> f16 image scaled by the query's own power of two (scan.h f16_shift)
        const float* row = reinterpret_cast<const float*>(A.Q) + (size_t)i * A.d;
        float amax = 0.f;
        for (int kk = lane; kk < A.d; kk += 64) amax = fmaxf(amax, fabsf(row[kk]));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        const int sh = f16_shift(amax);
        for (int kk = lane; kk < A.d; kk += 64) qimg[(size_t)i * A.d + kk] = (_Float16)ldexpf(row[kk], sh);
    }
    for (int j = lane; j < A.k; j += 64) A.D_out[(size_t)i * A.k + j] = out_score(-3.4028234663852886e38f, A.metric);   // "no bound known"
    double B, unscale, off;
    query_bound(A, i, i, lane, B, unscale, off);    // fills the cache (A.qb_ready == 0 here)
    if (seed != nullptr) l2_long_bound(A, i, lane, B, unscale, seed);       // (B stays the global bound: infinite or not is all the threshold asks)
    if (lane == 0) { qsel[i] = i; A.thr[i] = long_thr(A, -INFINITY, B); A.cnt[i] = 0u; A.status[i] = 1; }
}

// k_bound_prepare (sss_ip_topk_long, between two levels; scan.h: launch_bound_prepare): no row is read.  At least k of
// the kept rows have a scan score >= the k-th largest kept scan score s_k, so at least k rows have an exact score
// >= s_k * unscale - B: a valid LOWER BOUND of the query's true k-th score, written to column k-1 of its row of D_out
// (left unchanged when the kept rows overflowed the capacity or are fewer than k) -- and the next level's threshold
// straight from it (what k_thr_prepare would compute in a launch of its own).  The four radix passes run over LDS: read
// from the array in global memory they moved 4 x 64 KB per query -- 270 MB for the first level of a 1024-query search
// (every one of its 8192 sampled rows is kept), 70 us.  One workgroup per query; the selection by all of it, the rest
// by its first wave.
__global__ __launch_bounds__(SORT_THREADS) void k_bound_prepare(const ThrArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned* ords = reinterpret_cast<unsigned*>(smem);                 // [cap] score ordinals of the kept rows
    __shared__ unsigned s_hist[260];
    const int i = blockIdx.x, tid = threadIdx.x;
    const int q = A.qsel[i];
    const int k = A.k;
    const unsigned M = A.cnt[i];
    const bool have = M <= (unsigned)A.cap && (int)M >= k;              // (workgroup-uniform)
    unsigned sk = 0u;
    if (have) {
        const unsigned long long* ck = A.cand + (size_t)i * A.cap;
        for (int x = tid; x < (int)M; x += SORT_THREADS) ords[x] = (unsigned)(ck[x] >> 32);
        __syncthreads();
        sk = kth_largest_of<SORT_THREADS>([&](int x) { return ords[x]; }, (int)M, k, tid, s_hist);
    }
    if (tid >= 64) return;
    double B, unscale, off;
    query_bound(A, i, q, tid, B, unscale, off);
    float lbf = out_score(A.D_out[(size_t)q * k + k - 1], A.metric);    // (L2: the column holds an UPPER bound of the k-th distance)
    if (have) {
        const double lb = (double)ord2f(sk) * unscale + off - B;
        float f = (float)lb;
        if ((double)f > lb) f = nextafterf(f, -INFINITY);               // round DOWN: stays a lower bound
        if (f == f && f > lbf) { lbf = f; if (tid == 0) A.D_out[(size_t)q * k + k - 1] = out_score(f, A.metric); }
    }
    const float thr = long_thr(A, thr_from_bound((double)lbf, B, unscale, off), B);
    if (tid == 0) A.thr[i] = thr;
    if (!A.keep) {
        if (tid == 0) A.cnt[i] = 0u;
        return;
    }
    prune_kept(A, i, thr, tid);
}

// k_select_all: one workgroup per selected query.  The kept rows are first pruned by SCAN score, before any row is
// read: with s_k the k-th largest kept scan score, at least k rows have an exact score >= s_k * unscale - B, and a
// row whose scan score lies more than 2 B (+ one float32 ulp) below s_k cannot reach that -- the survivors are a
// superset of every possible result, typically k + a few.  They are re-scored canonically (float64, sequential in
// k, from the stored rows), bitonic-sorted by (score desc, id asc), the first k written.  status[q] = 0 when the
// kept rows fit the capacity (and there are at least min(k, n) of them); untouched otherwise.
// Launched twice: first with a SMALL LDS footprint (`cap_lds` = 2048 keys: several workgroups per CU -- the common
// case of a few hundred kept rows), then with the full capacity for the queries the first launch had to skip
// (`second`: resolved queries return at once).
template <int SA_ROWS>
__global__ __launch_bounds__(SORT_THREADS) void k_select_all(const ThrArgs A, int cap_pow2, int second) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);             // [cap_pow2] kept rows (scan keys)
    unsigned long long* surv = keys + cap_pow2;                                          // [cap_pow2] survivors, then exact keys
    char* qrow = reinterpret_cast<char*>(surv + cap_pow2);
    __shared__ unsigned s_hist[260];
    __shared__ float s_cut;
    __shared__ unsigned s_keep;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int q = A.qsel[i];
    const int rb = row_bytes(A.d, A.dtype);
    const int k = A.k;
    const unsigned M = A.cnt[i];
    const long need = (long)k < (long)A.n ? k : A.n;
    if (M > (unsigned)A.cap || (long)M < need) return;                  // overflow (or NaNs): stays unproven
    if (M > (unsigned)cap_pow2 || (second && A.status[q] == 0)) return; // the other launch's share
    load_query_row<SORT_THREADS>(qrow, A.Q, q, rb, tid);
    const unsigned long long* ck = A.cand + (size_t)i * A.cap;
    for (int c = tid; c < (int)M; c += SORT_THREADS) keys[c] = ck[c];
    if (tid == 0) { s_cut = -INFINITY; s_keep = 0u; }
    __syncthreads();
    if ((int)M > 2 * k + 64) {                                          // (worth a selection only when there is much to prune)
        const unsigned sk_o = kth_largest_ord(keys, (int)M, k, tid, s_hist);
        if (tid < 64) {
            double B, unscale, off;
            query_bound(A, i, q, tid, B, unscale, off);
            B = select_bound(A, i, B);
            if (tid == 0) {
                const double sk = (double)ord2f(sk_o);
                const double c = sk - (2.0 * B + ULP32_REL * fabs(sk * unscale + off) + ULP32_MIN) / unscale;
                float f = (float)c;
                if ((double)f > c) f = nextafterf(f, -INFINITY);
                s_cut = f == f ? f : -INFINITY;                         // (NaN bound: keep everything)
            }
        }
        __syncthreads();
    }
    const float cut = s_cut;
    for (int c = tid; c < (int)M; c += SORT_THREADS) {
        const unsigned long long key = keys[c];
        if (key_score(key) >= cut || !(cut > -INFINITY)) surv[atomicAdd(&s_keep, 1u)] = key;
    }
    __syncthreads();
    const int keep = (int)s_keep;                                       // >= k: the k-th largest itself passes the cut
    int K2 = 64;
    while (K2 < keep) K2 <<= 1;
    // canonical re-score of the survivors (rescore_kept: SA_ROWS rows at a time through the staging tile for long rows)
    char* stage = qrow + ((rb + 15) & ~15);                             // [SA_ROWS][SA_BYTES + 16]
    // (stored rows narrower than the scan, ThrArgs::d_row: a stored row of 1024 bytes or more implies a query row -- the
    //  host sizes the tile by it -- at least as long)
    rescore_kept<SA_ROWS>(surv, keep, K2, A.C, stored_row_bytes(A), rescore_type(A.dtype, A.metric), qrow, stage, tid,
                          [&](int c, bool valid, double acc, int id) __attribute__((always_inline)) {
                              keys[c] = valid ? make_key((float)acc, id) : 0ull;     // (the scan keys are no longer needed)
                          });
    __syncthreads();
    // Many more survivors than results (a query whose k-th neighbour sits in a group of thousands of identical rows: config
    // C3's one-click prefix sessions): a bitonic sort of all K2 exact keys -- 91 barrier stages at K2 = 8192 -- was 0.3 of
    // the 0.5 ms such a workgroup took.  The k best are SELECTED first (two radix descents: the k-th largest score ordinal,
    // then, inside its tie group, the id word that completes the count -- keys are unique, so exactly k lie at or above the
    // resulting key) and only they are sorted.
    int Ks = 64;
    while (Ks < k) Ks <<= 1;
    const unsigned long long* outk = keys;
    if (keep > 2 * Ks) {
        const unsigned long long T = kth_largest_key(keys, keep, k, tid, s_hist, &s_keep);
        __syncthreads();
        if (tid == 0) s_keep = 0u;
        __syncthreads();
        for (int x = tid; x < keep; x += SORT_THREADS) {                // (surv: the survivors' scan keys are no longer needed)
            const unsigned long long kx = keys[x];
            if (kx >= T) surv[atomicAdd(&s_keep, 1u)] = kx;
        }
        __syncthreads();
        for (int x = (int)s_keep + tid; x < Ks; x += SORT_THREADS) surv[x] = 0ull;
        __syncthreads();
        sort_desc(surv, Ks, tid);
        outk = surv;
    } else {
        sort_desc(keys, K2, tid);
    }
    float* Dq = A.D_out + (size_t)q * k;
    long* Iq = A.I_out + (size_t)q * k;
    for (int j = tid; j < k; j += SORT_THREADS) {
        if (j < keep) { Dq[j] = out_score(key_score(outk[j]), A.metric); Iq[j] = (long)key_id(outk[j]) + A.id_offset; }
        else pad_result(Dq, Iq, j, A.metric);
    }
    if (tid == 0) A.status[q] = 0;
}

// ------------------------------------------------------------------------------------------
// RANGE SEARCH, fused route (ip_topk.hip: sss_range_search_count / sss_range_search_fill).  The threshold rung with the caller's
// radius r in place of a known k-th score: a row the scan does NOT keep has scan score <= thr_from_bound(r), hence an
// exact score below r - one float32 ulp of r, which rounds to at most r -- never "> r".  So the rows kept are a superset
// of the answer, and re-scoring all of them canonically decides it exactly (when they fit the capacity).
//
// k_range_prepare: one wave per query (identity selection): its scan threshold from its radius, counter zeroed.
__global__ __launch_bounds__(256) void k_range_prepare(const ThrArgs A, const float* __restrict__ radius, int* __restrict__ qsel) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.nsel) return;
    double B, unscale, off;
    query_bound(A, i, i, lane, B, unscale, off);                            // (every lane ends up with the same B / unscale)
    const float thr = thr_from_bound((double)radius[i], B, unscale, off);        // -inf for r <= -3e38 (and NaN): keep every row
    if (lane == 0) { qsel[i] = i; A.thr[i] = thr; A.cnt[i] = 0u; }
}

// Range output entry of a kept row: (~id) in the high word, the float32 score's bits in the low one.  A DESCENDING sort
// of these orders by ASCENDING id (ids < 2^31: ~id >= 2^31), and 0 -- the padding -- sorts last.
__device__ __forceinline__ unsigned long long range_entry(float s, int id) {
    return ((unsigned long long)(~(unsigned)id) << 32) | (unsigned long long)__builtin_bit_cast(unsigned, s);
}

// k_range_select: one workgroup per query.  A query whose scan kept more rows than the capacity gets status 1 and count
// 0 (the exhaustive route resolves it).  Otherwise its M kept rows are re-scored canonically (rescore_kept), those with
// float32 score > radius are compacted in LDS, sorted by ascending id and written back over the query's candidate row
// of the workspace (for k_range_fill); cnt[i] and counts[i] = their number, status 0.
// Launched twice, as k_select_all: queries with m_lo < M <= cap_pow2 are this launch's share (the first launch, m_lo < 0,
// a small LDS footprint for the common case of a few hundred kept rows; it also flags the overflowed queries).
// LDS: keys[cap_pow2] scan keys | out[cap_pow2] entries | query row | staging tile (rows of 1024 bytes and more).
template <int SA_ROWS>
__global__ __launch_bounds__(SORT_THREADS) void k_range_select(const ThrArgs A, const float* __restrict__ radius, int cap_pow2, int m_lo,
                                                               long* __restrict__ counts, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem);
    unsigned long long* out = keys + cap_pow2;
    char* qrow = reinterpret_cast<char*>(out + cap_pow2);
    char* stage = qrow + ((row_bytes(A.d, A.dtype) + 15) & ~15);
    __shared__ unsigned s_keep;
    const int i = blockIdx.x, tid = threadIdx.x;
    const int rb = row_bytes(A.d, A.dtype);
    const unsigned M = A.cnt[i];
    if (M > (unsigned)A.cap) {                                          // overflow: the exhaustive route's
        if (m_lo < 0 && tid == 0) { counts[i] = 0; status[i] = 1; }
        return;
    }
    if ((int)M <= m_lo || M > (unsigned)cap_pow2) return;               // the other launch's share
    const float r = radius[i];
    load_query_row<SORT_THREADS>(qrow, A.Q, i, rb, tid);
    unsigned long long* ck = const_cast<unsigned long long*>(A.cand) + (size_t)i * A.cap;
    for (int c = tid; c < (int)M; c += SORT_THREADS) keys[c] = ck[c];
    if (tid == 0) s_keep = 0u;
    __syncthreads();
    int K2 = 64;
    while (K2 < (int)M) K2 <<= 1;                                       // <= cap_pow2
    rescore_kept<SA_ROWS>(keys, (int)M, K2, A.C, rb, A.dtype, qrow, stage, tid,
                          [&](int, bool valid, double acc, int id) __attribute__((always_inline)) {
                              const float s = (float)acc;
                              if (valid && s > r) {
                                  const unsigned pos = atomicAdd(&s_keep, 1u);
                                  if (pos < (unsigned)cap_pow2) out[pos] = range_entry(s, id);
                              }
                          });
    __syncthreads();
    const int keep = (int)min(s_keep, (unsigned)cap_pow2);              // (<= M: every kept row once)
    int Ks = 64;
    while (Ks < keep) Ks <<= 1;
    for (int x = keep + tid; x < Ks; x += SORT_THREADS) out[x] = 0ull;
    __syncthreads();
    sort_desc(out, Ks, tid);                                            // ascending id
    for (int x = tid; x < keep; x += SORT_THREADS) ck[x] = out[x];      // (the row's scan keys were read above)
    if (tid == 0) { A.cnt[i] = (unsigned)keep; counts[i] = keep; status[i] = 0; }
}

// k_range_fill: one workgroup per query: its resolved entries (cnt[i] <= cap) to D / I at lims[i], ids + id_offset.
// Writes stay inside [lims[i], lims[i+1]) and below lims[nq] (the size of D / I) whatever lims holds.
__global__ __launch_bounds__(256) void k_range_fill(const unsigned* __restrict__ cnt, const unsigned long long* __restrict__ cand,
                                                    int cap, int nq, const long* __restrict__ lims, long id_offset,
                                                    float* __restrict__ D, long* __restrict__ I) {
    const int i = blockIdx.x;
    const unsigned m = cnt[i];
    if (m > (unsigned)cap) return;                                      // overflowed: filled by the exhaustive route
    const long total = lims[nq], lo = lims[i], hi = lims[i + 1];
    if (lo < 0 || lo > total) return;
    long len = (long)m;
    if (hi - lo < len) len = hi - lo;
    if (total - lo < len) len = total - lo;
    const unsigned long long* row = cand + (size_t)i * cap;
    for (long j = threadIdx.x; j < len; j += 256) {
        const unsigned long long e = row[j];
        D[lo + j] = __builtin_bit_cast(float, (unsigned)e);
        I[lo + j] = (long)(int)~(unsigned)(e >> 32) + id_offset;
    }
}

// ------------------------------------------------------------------------------ host side
int launch_thr_prepare(const ThrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_thr_prepare, dim3((unsigned)((a.nsel + 3) / 4)), dim3(256), 0, st, a);
    return check_launch("k_thr_prepare");
}

int launch_long_setup(const ThrArgs& a, int* qsel, void* qimg, float* seed, hipStream_t st) {
    hipLaunchKernelGGL(k_long_setup, dim3((unsigned)((a.nsel + 3) / 4)), dim3(256), 0, st, a, qsel, reinterpret_cast<_Float16*>(qimg), seed);
    return check_launch("k_long_setup");
}

int launch_bound_prepare(const ThrArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_bound_prepare, dim3((unsigned)a.nsel), dim3(SORT_THREADS), (size_t)a.cap * 4, st, a);     // (cap <= 8192: 32 KB)
    return check_launch("k_bound_prepare");
}

// LDS sizing of the kernels launched twice (k_select_all, k_range_select): a first launch with room for `small` kept rows
// (<= 2048: several workgroups per CU -- the common case of a few hundred kept rows), then one with the full capacity
// cap_pow2 for the queries the first had to skip.  lds(c, tile) = two key arrays of c + the query row + `tile` bytes of
// staging (rows of 1024 bytes and more; shorter rows are walked by a thread each).
struct TwoLaunchLds {
    int rb, cap_pow2, small;
    size_t row, stage_full;
    size_t lds(int c, size_t tile) const { return 2 * (size_t)c * 8 + row + tile; }
};
static int two_launch_lds(const ThrArgs& a, const char* what, TwoLaunchLds& s) {
    s.rb = a.d * elem_bytes(a.dtype);
    s.cap_pow2 = pow2_at_least(a.cap);
    s.small = s.cap_pow2 < 2048 ? s.cap_pow2 : 2048;
    s.row = (s.rb + 15) & ~15;
    s.stage_full = s.rb < 1024 ? 0 : (size_t)SA_ROWS_FULL * (SA_BYTES + 16);
    if (s.lds(s.cap_pow2, s.stage_full) <= 156 * 1024) return SSS_OK;
    set_error("%s: candidate capacity %d / row of %d bytes too large", what, a.cap, s.rb);
    return SSS_EINVAL;
}

int launch_select_all(const ThrArgs& a, hipStream_t st) {
    TwoLaunchLds s;
    int rc = two_launch_lds(a, "select_all", s);
    if (rc) return rc;
    const size_t stage_small = s.rb < 1024 ? 0 : (size_t)SA_ROWS_SMALL * (SA_BYTES + 16);
    rc = opt_in_lds(reinterpret_cast<const void*>(&k_select_all<SA_ROWS_SMALL>), "k_select_all", 160 * 1024 - 4096);
    if (!rc) rc = opt_in_lds(reinterpret_cast<const void*>(&k_select_all<SA_ROWS_FULL>), "k_select_all", 160 * 1024 - 4096);
    if (rc) return rc;
    // (k <= 64: k + a few dozen survivors fit one 128-row group, and a 256-row group would fetch twice the clamped copies)
    if (a.k > 64) hipLaunchKernelGGL(k_select_all<SA_ROWS_SMALL>, dim3((unsigned)a.nsel), dim3(SORT_THREADS), s.lds(s.small, stage_small), st, a, s.small, 0);
    else hipLaunchKernelGGL(k_select_all<SA_ROWS_FULL>, dim3((unsigned)a.nsel), dim3(SORT_THREADS), s.lds(s.small, s.stage_full), st, a, s.small, 0);
    if (s.small < s.cap_pow2) hipLaunchKernelGGL(k_select_all<SA_ROWS_FULL>, dim3((unsigned)a.nsel), dim3(SORT_THREADS), s.lds(s.cap_pow2, s.stage_full), st, a, s.cap_pow2, 1);
    return check_launch("k_select_all");
}

int launch_range_prepare(const ThrArgs& a, const float* radius, int* qsel, hipStream_t st) {
    hipLaunchKernelGGL(k_range_prepare, dim3((unsigned)((a.nsel + 3) / 4)), dim3(256), 0, st, a, radius, qsel);
    return check_launch("k_range_prepare");
}

int launch_range_select(const ThrArgs& a, const float* radius, long* counts, int* status, hipStream_t st) {
    TwoLaunchLds s;
    int rc = two_launch_lds(a, "range_select", s);
    if (!rc) rc = opt_in_lds(reinterpret_cast<const void*>(&k_range_select<SA_ROWS_FULL>), "k_range_select", 160 * 1024 - 4096);
    if (rc) return rc;
    hipLaunchKernelGGL(k_range_select<SA_ROWS_FULL>, dim3((unsigned)a.nsel), dim3(SORT_THREADS), s.lds(s.small, s.stage_full), st, a, radius,
                       s.small, -1, counts, status);
    rc = check_launch("k_range_select");
    if (rc || s.small == s.cap_pow2) return rc;
    hipLaunchKernelGGL(k_range_select<SA_ROWS_FULL>, dim3((unsigned)a.nsel), dim3(SORT_THREADS), s.lds(s.cap_pow2, s.stage_full), st, a, radius,
                       s.cap_pow2, s.small, counts, status);
    return check_launch("k_range_select");
}

int launch_range_fill(const unsigned* cnt, const unsigned long long* cand, int cap, long nq, const long* lims, long id_offset, float* D,
                      long* I, hipStream_t st) {
    hipLaunchKernelGGL(k_range_fill, dim3((unsigned)nq), dim3(256), 0, st, cnt, cand, cap, (int)nq, lims, id_offset, D, I);
    return check_launch("k_range_fill");
}

}  // namespace sss
