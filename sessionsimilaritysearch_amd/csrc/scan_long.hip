// Scoring + top-k for LONG rows -- the reference's own session vectors are D = 1600 wide with K = 100
// (pretrain_filtered_amazon.py:281, test_amazon_filterd.py:459,578: `index.search(normalize(emb), K)`), far beyond
// the 1024-byte rows k_scan keeps resident in registers.  gfx950 / CDNA4.
//
// A row of 3200 bytes (f16 image of a float32 index) or more fits neither the registers nor LDS next to a query
// tile, so the scan is a K-TILED contraction: k_scan_long = 256 queries x 256 corpus rows per workgroup tile,
// both operands streamed through LDS in 128-byte K slabs (LDS-DMA, double buffered, XOR swizzle on the source
// address), v_mfma_f32_32x32x16_{f16,bf16} accumulating the full dot products in 8 accumulators per wave
// (a wave = 64 queries x 128 rows: two B operands x four row blocks; a lane owns one query column per operand).
//
// The top-k rides on the THRESHOLD machinery of the rung (select_thr.hip: THRESHOLD RUNG) instead of running lists:
// the epilogue of a tile only compares its 128 scores per lane with the lane's fixed threshold and appends what
// passes.  The threshold comes from LEVELS of evenly spread row samples:
//   level 1   a sample of up to `cap` rows (>= 2k), threshold -inf: every sampled row is kept; at least k of them have a scan
//             score >= the k-th largest kept scan score s_k, hence an exact score >= s_k - (scan error bound): a
//             valid LOWER BOUND of the true k-th score (k_bound_prepare: a selection over scan scores, no row is read);
//   level i   a sample r <= `fmax` times larger scanned with threshold = (bound - error bound - one ulp): about
//             k * fmax rows pass per query -> a tighter bound the same way;
//   last      every row.  What passes is everything that can still reach the k-th score already known -- near ties
//             and duplicate rows included -- so the canonical float64 re-score of all of it (k_select_all) IS the
//             exact answer (status 0); a query with more than 8192 such rows keeps status 1 and goes to the
//             exhaustive kernels.  The last sample is 1/r of the corpus: ~r k rows per query reach the re-score.
//   With three levels and more the last sample and the final level are DISJOINT (host side, "DISJOINT LEVELS"): the
//   sample takes every R-th tile, the final level the tiles in between, and the rows the sample kept stay (pruned in place
//   to the final threshold) -- no tile is scanned twice.
// Two to three passes, the last one dominant; no per-lane list, no shared threshold slots, no bootstrap.
#include "scan.h"
#include <algorithm>
#include <cmath>
#include "scan_dev.h"

namespace sss {

constexpr int LT_ROWS = 256;        // corpus rows per workgroup tile
constexpr int LT_Q = 256;           // queries per workgroup (8 waves x 32)
constexpr int LT_BK = 128;          // bytes of K per slab (64 16-bit elements = 4 MFMA k-groups)
constexpr int LT_HALF = LT_ROWS * LT_BK;               // 32 KB: one slab of ONE operand (LT_ROWS == LT_Q)
// LDS: the corpus slabs in a ring of THREE, the query slabs in a ring of two -- all 160 KB.  The corpus slab (streamed
// from HBM: the long latency) is fetched two slabs ahead, the query slab (L2-resident) one: half the bytes that must
// land within one slab's matrix time, and the far operand gets the deep look-ahead (counters, round 4: the waves were
// parked 52 % of their cycles waiting for the single 64 KB slab in flight; L2 hit rate 71 %, fetch from HBM ~1.2x
// algorithmic, no LDS stall or conflict -- the bound was the latency of a one-slab look-ahead, not a rate).
constexpr int LT_LDS_BYTES = 5 * LT_HALF;
static_assert(LT_ROWS == LT_Q, "the two operand slabs have one size");

struct LongArgs {
    const void* Qimg;               // [nq][d] 16-bit queries (f16 image of f32 queries; bf16 / f16 index: the queries themselves)
    const void* C;                  // [n][d] 16-bit rows (f16 image of f32 rows; bf16 / f16 rows)
    int nq, n, d, G, S;
    int gpx;                        // query groups that share an XCD (block map below); divides G, G / gpx divides 8
    int dense;                      // sample level (many rows kept per lane and tile): aggregated appends
    int tile_count;                 // tiles this level scans: tile j of the level = corpus tile j * total_tiles / tile_count
    int skip_R;                     // > 0: the level scans the tile_count corpus tiles that are NOT multiples of skip_R, in order
                                    //      (the complement of a level that took every skip_R-th tile: DISJOINT LEVELS, host side)
    int total_tiles, tiles_per_split, cap;
    const float* thr;               // [nq] per-query threshold in the scan's domain
    unsigned* cnt;                  // [nq] rows kept so far
    unsigned long long* cand;       // [nq][cap]
    // L2 scans only (k_scan_long<DT_F16, MET = 1>; appended, so the inner-product kernels read what they always read): the
    // per-row bias -|c|^2 / 2 every score starts from, and per query the two coefficients of the seed (k_long_setup;
    // select_thr.hip: THE PER-ROW BOUND): seed[row] = seed[0][q] * bias[row] + seed[1][q] * |c_row|.  seed[0] is sigma (the
    // power of two the query's scaled scores live in) times (1 +- Q), seed[1] = -+ sigma P / 2: the key comes out LOWERED
    // by the row's own error bound on the sample levels and RAISED by it on the last level.
    const float* bias = nullptr;    // [n]
    const float* seed = nullptr;    // [2][nq]
};

// (the f16 image of f32 queries -- scaled by the query's own power of two, scan.h: f16_shift -- is written by
//  select_thr.hip: k_long_setup; the select side, query_bound / k_thr_prepare, re-derives the same shift)

constexpr int LT_LOADERS = 4;                          // loader waves per workgroup (one per SIMD), behind the 8 matrix waves
constexpr int LT_NP = 32 / LT_LOADERS;                 // 1 KiB pieces of an operand slab per loader
constexpr int LT_THREADS = (8 + LT_LOADERS) * 64;

// MET = 1 is the L2 form (as k_scan's, scan_kernel.h): the key of (query, row) is sigma (q.c) + seed[row] -- every
// accumulator of a tile starts from its rows' seeds instead of zero, landed in the accumulator layout by one
// v_mfma_f32_32x32x2_f32 per accumulator (A = the 32 rows' biases in the k = 0 column and their norms |c| in k = 1;
// B = the lane's query's two seed coefficients), and everything from the K loop to the appends runs as before.  The
// inner-product instantiations (MET = 0) compile to what they were: every L2 statement sits under `if constexpr (MET)`.
template <int DT, int MET = 0>
__global__ __launch_bounds__(LT_THREADS, (LT_THREADS + 255) / 256) void k_scan_long(const LongArgs A) {
    static_assert(DT == DT_F16 || DT == DT_BF16, "16-bit rows");
    static_assert(MET == 0 || DT == DT_F16, "an L2 index is float32: its long scan reads the scaled f16 image");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nq = A.nq, n = A.n, S = A.S, G = A.G;
    const int rb = A.d * 2;                             // bytes per row (queries and corpus alike)
    const int nslab = rb / LT_BK;
    const char* __restrict__ Qb = reinterpret_cast<const char*>(A.Qimg);
    const char* __restrict__ Cb = reinterpret_cast<const char*>(A.C);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, h = lane >> 5;

    // XCD-aware block map: the G query groups that stream one corpus split sit on ONE XCD (blocks b and b + 8 share an
    // XCD and its L2: the split is fetched from HBM once and re-read from that L2 by the other groups; speed only, never
    // correctness).  gpx < G -- an XCD serving fewer groups and more splits, so that its query images (800 KB a group
    // at d = 1600) stay L2-resident -- was measured in round 4: 1-4 % SLOWER (L2 hit rate 71 % as it is; the queries
    // are not what misses), so the plan keeps gpx = G.
    const int bid = blockIdx.x;
    const int xcd = bid & 7, slot = bid >> 3;
    const int gpx = A.gpx, nteam = G / gpx;                       // XCD teams: team t serves groups [t gpx, (t + 1) gpx)
    const int team = xcd % nteam, xi = xcd / nteam;               // this XCD's team and its index inside the team
    const int splits_per_xcd = (S * G >> 3) / gpx;
    const int split = xi * splits_per_xcd + slot / gpx;
    const int g = team * gpx + slot % gpx;
    int j_lo = split * A.tiles_per_split, j_hi = j_lo + A.tiles_per_split;
    if (j_hi > A.tile_count) j_hi = A.tile_count;
    if (j_lo >= j_hi) return;                           // whole workgroup: no barrier below is skipped by part of it

    const int total_steps = (j_hi - j_lo) * nslab;             // slab steps of this split
    // tile j of the level = corpus tile floor(j * total_tiles / tile_count), advanced incrementally (one division here
    // instead of a 64-bit scalar division sequence per tile)
    // (skip_R > 0: the j-th tile that is not a multiple of R is (j / (R - 1)) R + 1 + j % (R - 1); `tile_frac` then holds
    //  tile % R and a step that lands on a multiple of R moves one further)
    const int skip_R = A.skip_R;
    const int t_quo = A.total_tiles / A.tile_count, t_rem = A.total_tiles % A.tile_count;
    int tile = skip_R > 0 ? (j_lo / (skip_R - 1)) * skip_R + 1 + j_lo % (skip_R - 1) : (int)((long)j_lo * A.total_tiles / A.tile_count);
    int tile_frac = skip_R > 0 ? 1 + j_lo % (skip_R - 1) : (int)((long)j_lo * A.total_tiles % A.tile_count);
    auto next_tile = [&](int& tl, int& fr) __attribute__((always_inline)) {
        if (skip_R > 0) {
            ++tl;
            if (++fr == skip_R) { fr = 1; ++tl; }
            return;
        }
        tl += t_quo; fr += t_rem;
        if (fr >= A.tile_count) { fr -= A.tile_count; ++tl; }
    };

    // ---- LDS: a slab is [256 rows][128 B] of one operand in 1 KiB pieces (8 rows x 8 chunks); chunk c of row t sits
    // at chunk slot c ^ ((t >> 1) & 7): with 128-byte rows two rows share a 256-byte bank row, and this key makes every
    // 16-lane group of a ds_read_b128 (16 consecutive rows, one chunk) cover all 64 banks exactly once.  Corpus slabs
    // in a ring of three slots, query slabs in a ring of two behind them.
    // Steps run over (tile, slab) pairs; step t reads corpus slot t % 3 and query slot t % 2; ONE barrier per step.
    //
    // LOADER WAVES (round 4).  Twelve waves: eight matrix waves and four loaders, one per SIMD.  A DMA instruction costs
    // its wave 100-200 cycles of issue in this loop (MI355X_MICROARCH.md, LDS-DMA piece issue cost) -- with every wave
    // issuing its eight pieces of each slab, ~1.2 k cycles per wave and slab in which it issued no matrix instruction,
    // against 1 k of its own matrix work: the pipe was 43 % busy with the waves parked half of their time.  Here the
    // matrix waves issue NO vector-memory instruction inside the K loop (their counter only sees the tile epilogue's
    // stores), the loaders nothing else: sixteen pieces per loader and step -- the query pieces of step t + 1, then the
    // corpus pieces of step t + 2 -- and `vmcnt(8)` at the top of a step leaves exactly the youngest eight (corpus,
    // t + 2) in flight while everything step t + 1 reads is known to have landed before the barrier releases it.
    const unsigned lds_base = (unsigned)(unsigned long)(lptr_c)smem;
    if (wave >= 8) {
        const int lw = wave - 8;
        unsigned off_q[LT_NP], off_c[LT_NP];
        const char* q_base = Qb + (size_t)g * LT_Q * rb;
        const char* c_base = Cb;
#pragma unroll
        for (int i = 0; i < LT_NP; ++i) {
            const int t = ((lw + LT_LOADERS * i) << 3) + (lane >> 3);    // query row of the tile: piece lw + 4 i
            int tq = t;
            if (g * LT_Q + tq > nq - 1) tq = nq - 1 - g * LT_Q;          // short query batch: clamp (the group holds >= 1 query)
            off_q[i] = (unsigned)tq * (unsigned)rb + (unsigned)(((lane & 7) ^ ((t >> 1) & 7)) * 16);
        }
        auto set_tile = [&](int tl) __attribute__((always_inline)) {
            c_base = Cb + (size_t)tl * LT_ROWS * rb;
#pragma unroll
            for (int i = 0; i < LT_NP; ++i) {
                const int t = ((lw + LT_LOADERS * i) << 3) + (lane >> 3);   // corpus row of the tile
                int tc = t;
                if ((long)tl * LT_ROWS + tc > (long)n - 1) tc = (int)((long)n - 1 - (long)tl * LT_ROWS);   // ragged last tile: clamp
                off_c[i] = (unsigned)tc * (unsigned)rb + (unsigned)(((lane & 7) ^ ((t >> 1) & 7)) * 16);
            }
        };
        // one operand slab: a uniform 64-bit base (first row + slab offset: scalar adds) and per-lane 32-bit offsets
        auto stage = [&](const char* base, const unsigned (&off)[LT_NP], int slot_idx, int slab) __attribute__((always_inline)) {
            const unsigned long bv = (unsigned long)(base + (size_t)slab * LT_BK);
            // (readfirstlane returns int: without the unsigned casts a low word with bit 31 set sign-extends into the high word)
            const unsigned long bs = ((unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)(bv >> 32)) << 32) | (unsigned long)(unsigned)__builtin_amdgcn_readfirstlane((int)bv);
#pragma unroll
            for (int i = 0; i < LT_NP; ++i) {
                const unsigned dst = __builtin_amdgcn_readfirstlane(lds_base + slot_idx * LT_HALF + (lw + LT_LOADERS * i) * 1024);
                lds_dma16(off[i], dst, bs);
            }
        };
        int itile = tile, ifrac = tile_frac, islab = 0, ibuf = 0;   // next corpus slab to fetch and its ring slot
        auto issue_rows = [&]() __attribute__((always_inline)) {
            if (islab == 0) set_tile(itile);
            stage(c_base, off_c, ibuf, islab);
            ibuf = ibuf == 2 ? 0 : ibuf + 1;
            if (++islab == nslab) { islab = 0; next_tile(itile, ifrac); }
        };
        issue_rows();
        stage(q_base, off_q, 3, 0);
        if (total_steps > 1) issue_rows();
        int qslab = 1 % nslab;                                      // query slab of step + 1
        static_assert(LT_NP == 8, "the wait below leaves one corpus slab's pieces of this loader in flight");
        for (int step = 0; step < total_steps; ++step) {
            if (step + 2 > total_steps - 1) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");    // all but the youngest LT_NP pieces (corpus, step + 2)
            __syncthreads();                                        // step's slabs are there; the slots of step - 1 are free
            if (step + 1 < total_steps) stage(q_base, off_q, 3 + ((step & 1) ^ 1), qslab);
            if (step + 2 < total_steps) issue_rows();               // into slot (step + 2) % 3, read last in step - 1
            qslab = qslab + 1 == nslab ? 0 : qslab + 1;
        }
        return;                                                     // (the matrix waves' epilogues hold no barrier)
    }

    // ---- matrix waves: 4 query groups of 64 (two MFMA B operands: queries r and 32 + r of the group) x 2 halves of
    // the row tile (128 rows = four 32-row blocks): every fragment read from LDS feeds two MFMAs (24 ds_read_b128 per
    // slab and wave for 32 MFMAs; 32 queries x 256 rows per wave would need 36)
    const int wq = wave & 3, wr = wave >> 2;
    const int q0 = g * LT_Q + wq * 64 + r, q1 = q0 + 32;
    const float thr0 = q0 < nq ? A.thr[q0] : INFINITY;          // padding lanes never keep anything
    const float thr1 = q1 < nq ? A.thr[q1] : INFINITY;
    const f32x16 zero = {0};
    f32x16 acc[4][2];
    const int keyq0 = ((wq * 64 + r) >> 1) & 7, keyq1 = ((wq * 64 + 32 + r) >> 1) & 7;
    int step = 0, bufa = 0;                                     // bufa = step % 3
    // L2: bias of row (128 wr + 32 b + r) of the current tile in the lanes h = 0 (the k = 0 column of the seeding MFMA's A
    // operand); the lanes h = 1 hold its k = 1 column: an upper bound of the row's norm, sqrt(-2 bias) (1 + 2^-20) (the
    // bias is -|c|^2 / 2 rounded once; the factor covers that rounding and the square root's).  Rows at and beyond n read
    // row n - 1's and are masked by the epilogue's `row < n` like every other score of such a row.  The K loop issues no
    // vector-memory instruction in these waves, so a tile's four biases are fetched in the epilogue of the tile before
    // (the first tile's here) and waited for where they are used.  The coefficients are finite (k_long_setup).
    [[maybe_unused]] float bcur[MET ? 4 : 1];
    [[maybe_unused]] float sig0 = 1.f, sig1 = 1.f;
    [[maybe_unused]] auto bias_fetch = [&](int tl) __attribute__((always_inline)) {
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            long row = (long)tl * LT_ROWS + wr * 128 + b * 32 + r;
            if (row > (long)n - 1) row = (long)n - 1;
            const float bv = A.bias[row];
            bcur[b] = h == 0 ? bv : sqrtf(-2.f * bv) * 1.000001f;
        }
    };
    if constexpr (MET) {
        sig0 = q0 < nq ? A.seed[(size_t)h * nq + q0] : 0.f;
        sig1 = q1 < nq ? A.seed[(size_t)h * nq + q1] : 0.f;
        bias_fetch(tile);
    }
    for (int j = j_lo; j < j_hi; ++j) {
        if constexpr (MET) {
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                acc[b][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(bcur[b], sig0, zero, 0, 0, 0);
                acc[b][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(bcur[b], sig1, zero, 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b) { acc[b][0] = zero; acc[b][1] = zero; }
        }
        for (int s = 0; s < nslab; ++s, ++step) {
            const int bufb = step & 1;
            __syncthreads();                                    // the loaders have seen this step's slabs land
            const char* rows = smem + bufa * LT_HALF;
            const char* qs = smem + (3 + bufb) * LT_HALF;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 b0 = *reinterpret_cast<const f32x4*>(qs + (wq * 64 + r) * LT_BK + ((2 * u + h) ^ keyq0) * 16);
                const f32x4 b1 = *reinterpret_cast<const f32x4*>(qs + (wq * 64 + 32 + r) * LT_BK + ((2 * u + h) ^ keyq1) * 16);
                f32x4 a[4];
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int t = wr * 128 + b * 32 + r;
                    a[b] = *reinterpret_cast<const f32x4*>(rows + t * LT_BK + ((2 * u + h) ^ ((t >> 1) & 7)) * 16);
                }
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if constexpr (DT == DT_F16) {
                        acc[b][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[b]), __builtin_bit_cast(f16x8, b0), acc[b][0], 0, 0, 0);
                        acc[b][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a[b]), __builtin_bit_cast(f16x8, b1), acc[b][1], 0, 0, 0);
                    } else {
                        acc[b][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[b]), __builtin_bit_cast(bf16x8, b0), acc[b][0], 0, 0, 0);
                        acc[b][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a[b]), __builtin_bit_cast(bf16x8, b1), acc[b][1], 0, 0, 0);
                    }
                }
            }
            bufa = bufa == 2 ? 0 : bufa + 1;
        }
        if constexpr (MET) {                                    // the next tile's biases (this tile's are dead: it has been seeded)
            if (j + 1 < j_hi) {
                int ntile = tile, nfrac = tile_frac;
                next_tile(ntile, nfrac);
                bias_fetch(ntile);
            }
        }
        // ---- tile epilogue: acc[b][s][jj] is (corpus row tile * 256 + 128 wr + 32 b + (jj & 3) + 8 (jj >> 2) + 4 h,
        // query r (s = 0) / 32 + r (s = 1) of the wave's 64)
        const int qs[2] = {q0, q1};
        const float thrs[2] = {thr0, thr1};
        float m0 = -INFINITY, m1 = -INFINITY;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
#pragma unroll
            for (int jj = 0; jj < 16; jj += 2) {
                m0 = vmax3(m0, acc[b][0][jj], acc[b][0][jj + 1]);
                m1 = vmax3(m1, acc[b][1][jj], acc[b][1][jj + 1]);
            }
        }
        if (!A.dense) {
            // the last level: a lane keeps a row of a tile now and then -- one atomic add per kept row
            if (__builtin_amdgcn_ballot_w64(m0 > thr0 || m1 > thr1) != 0) {
                const int row_base = tile * LT_ROWS + wr * 128 + 4 * h;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
#pragma unroll
                    for (int jj = 0; jj < 16; ++jj) {
                        const int row = row_base + 32 * b + acc_row(jj);
#pragma unroll
                        for (int s = 0; s < 2; ++s) {
                            if (acc[b][s][jj] > thrs[s] && row < n) {
                                const unsigned pos = atomicAdd(A.cnt + qs[s], 1u);
                                if (pos < (unsigned)A.cap) A.cand[(size_t)qs[s] * A.cap + pos] = make_key(acc[b][s][jj], row);
                            }
                        }
                    }
                }
            }
        } else if (__builtin_amdgcn_ballot_w64(m0 > thr0 || m1 > thr1) != 0) {
            // The sample levels keep many rows per lane and tile (the first one EVERY row: threshold -inf) -- one atomic
            // add per lane and query for all of them (count, reserve, store); one per row made the first level cost
            // four times its matrix work.  (On the last level the counting pass costs more than it saves: +9 %.)
            const int row_base = tile * LT_ROWS + wr * 128 + 4 * h;
            unsigned cnt[2] = {0u, 0u}, at[2] = {0u, 0u};
#pragma unroll
            for (int b = 0; b < 4; ++b) {
#pragma unroll
                for (int jj = 0; jj < 16; ++jj) {
                    const bool in = row_base + 32 * b + acc_row(jj) < n;
#pragma unroll
                    for (int s = 0; s < 2; ++s) cnt[s] += (acc[b][s][jj] > thrs[s] && in) ? 1u : 0u;
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
                if (cnt[s]) at[s] = atomicAdd(A.cnt + qs[s], cnt[s]);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                unsigned long long* c = A.cand + (size_t)qs[s] * A.cap;
                if (__builtin_amdgcn_ballot_w64(cnt[s] != 0u) != 0) {
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
#pragma unroll
                        for (int jj = 0; jj < 16; ++jj) {
                            const int row = row_base + 32 * b + acc_row(jj);
                            if (acc[b][s][jj] > thrs[s] && row < n) {
                                if (at[s] < (unsigned)A.cap) c[at[s]] = make_key(acc[b][s][jj], row);
                                ++at[s];
                            }
                        }
                    }
                }
            }
        }
        next_tile(tile, tile_frac);
    }
}

// ------------------------------------------------------------------------------ host side
// What the scan reads for rows of `exact_dtype`: f32 rows their scaled f16 image, bf16 and f16 rows themselves (an f16
// index is its own image: shift 0, no residual, the f16 kernel as it is).
static int long_scan_dtype(int exact_dtype) { return exact_dtype == DT_F32 ? DT_F16 : exact_dtype; }
constexpr int LONG_CAP = 8192;      // rows kept per query (k_select_all sorts them in 64 KB of LDS)
constexpr int LONG_MAX_K = 1024;    // what the exhaustive kernels -- the path of a query left at status 1 -- can resolve
// k_select_all keeps 2 x cap keys + the exact query row + its staging tile in LDS: rows beyond 10240 bytes
// (f32 d > 2560, bf16 d > 5120) leave room for half the capacity only.
static int long_cap(int d, int exact_dtype) { return d * elem_bytes(exact_dtype) > 10240 ? LONG_CAP / 2 : LONG_CAP; }

// The workspace, written ONCE (offsets in bytes, every array 256-byte aligned): qimg 16-bit [nq][d] the f16 query image |
// qsel i32 [nq] the identity selection | thr f32 [nq] | cnt u32 [nq] | L2 only: seed f32 [2][2][nq], the seed coefficients
// for lowered, then for raised keys | qb f64 [nq][2] (error bound, unscale) per query, computed once; L2: + [nq] off = -|q|^2
// + [nq] the select's bound | cand u64 [nq][LONG_CAP].  cand is sized by LONG_CAP whatever the rows, as the sizing functions
// always have: a search whose long_cap(d, dtype) is half of it lays its [nq][cap] rows out in the first half of the array.
struct LongLayout { size_t qimg, qsel, thr, cnt, seed, qb, cand, total; };
static LongLayout long_layout(long nq, int d, bool l2) {
    LongLayout l;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t off = at; at += al256(bytes); return off; };
    l.qimg = take((size_t)nq * d * 2); l.qsel = take((size_t)nq * 4); l.thr = take((size_t)nq * 4); l.cnt = take((size_t)nq * 4);
    l.seed = l2 ? take((size_t)nq * 16) : 0;
    l.qb = take((size_t)nq * (l2 ? 32 : 16));
    l.cand = at; l.total = at + (size_t)nq * LONG_CAP * 8;
    return l;
}

extern "C" size_t sss_ip_topk_long_workspace_bytes(int64_t nq, int64_t n, int d, int dtype) {
    if (nq <= 0 || n <= 0 || !long_shape_ok(d, dtype, long_scan_dtype(dtype))) return 0;
    return long_layout(nq, d, false).total;
}

extern "C" size_t sss_l2_topk_long_workspace_bytes(int64_t nq, int64_t n, int d) {      // (include/sss_l2_long.h)
    if (nq <= 0 || n <= 0 || !long_shape_ok(d, DT_F32, DT_F16)) return 0;
    return long_layout(nq, d, true).total;
}

// One level of a search: a launch of k_scan_long over tile_count tiles (LongArgs: tile_count, total_tiles, skip_R, S,
// tiles_per_split, dense) and, behind every level but the last, the bound step with ThrArgs::keep.
struct LongLevel { int tile_count, total_tiles, skip_R, S, tiles_per_split, dense, keep; };
struct LongPlan { int levels = 0; LongLevel level[40]; };        // in the order they run: the samples growing, every row last

// The level schedule of a corpus of total_tiles tiles for G query groups: arithmetic on these integers, nothing else.
static LongPlan long_plan(int total_tiles, int cap, int k, bool l2, int G) {
    // ---- levels (descending in level_tiles, run in reverse).  The first sample is as large as the capacity allows with
    // the threshold at -inf (cap rows: every sampled row is kept) -- a 32-tile level costs the time of ONE tile, the chip
    // being far from full, and its k-th best score is a much better bound than that of a 2k-row sample.  From there to
    // the whole corpus the tile counts grow by equal factors r <= fmax = cap / (4 k): about k * r rows pass a level's
    // threshold (2x margin below the capacity at r = fmax), the fewest levels that allows, and the factors balanced so
    // that the last sample is as small as it can be (1M x 1600, K = 100: 32, 353, 3907 tiles -- the samples add ~10 % to
    // the matrix work; it was 1, 24, 488, 3907).  Intermediate levels read no row at all (k_bound_prepare).
    const int fmax = std::max(cap / (4 * k), 2), first = std::min(cap / LT_ROWS, total_tiles);
    int level_tiles[40];
    int levels = 0;
    level_tiles[levels++] = total_tiles;
    if (first < total_tiles) {
        const double span = (double)total_tiles / (double)first;
        int steps = 1;
        while (pow((double)fmax, (double)steps) < span && steps < 36) ++steps;      // growth steps from `first` to the corpus
        const double r = pow(span, 1.0 / (double)steps);
        for (int i = steps - 1; i >= 1; --i) {
            int tl = (int)((double)first * pow(r, (double)i) + 0.5);
            if (tl <= first) break;
            if (tl < level_tiles[levels - 1]) level_tiles[levels++] = tl;
        }
        level_tiles[levels++] = first;
    }
    // DISJOINT LEVELS (three levels and more).  The last sample used to be scanned twice: once as a sample, once more as
    // part of the whole corpus -- 9 % of the matrix work at 1M x 1600, K = 100.  Now the last sample takes EVERY R-th
    // tile (R = the planned ratio, rounded, >= 2) and the final level only the tiles in between: the rows the sample kept
    // stay in the query's array, pruned by k_thr_prepare to those that pass the final threshold (its `keep` mode; the
    // final threshold is the tighter one, so nothing above it was ever dropped), and the final level appends behind
    // them.  Together they are exactly the rows of the whole corpus above the final threshold -- what k_select_all's
    // proof needs -- and there are fewer of them (the sample's rows are filtered by the final threshold now).
    // Never for L2: a sample's kept rows carry lowered keys, which the final threshold (made for raised keys) must not prune.
    int R = 0;
    if (levels >= 3 && !l2) {
        R = (int)((double)total_tiles / (double)level_tiles[1] + 0.5);
        if (R < 2) R = 0;                              // (ratio below 1.5: the planned sample is most of the corpus -- keep the plain form)
    }
    LongPlan p;
    for (int lv = levels - 1; lv >= 0; --lv) {
        LongLevel& v = p.level[p.levels++];
        const bool last = lv == 0, last_sample = R > 0 && lv == 1;
        v.tile_count = level_tiles[lv]; v.total_tiles = total_tiles; v.skip_R = 0;
        if (last_sample) {                             // every R-th tile: the proportional map with total = R * count
            v.tile_count = (total_tiles + R - 1) / R;
            v.total_tiles = R * v.tile_count;
        } else if (R > 0 && last) {                    // the tiles in between
            v.tile_count = total_tiles - (total_tiles + R - 1) / R;
            v.skip_R = R;
        }
        v.dense = last ? 0 : 1;
        v.keep = last_sample ? 1 : 0;                  // the final level keeps this (the last sample's) rows that pass its thresholds
        v.S = std::max((256 / G) & ~7, 8);
        while (v.S > 8 && v.S > v.tile_count) v.S -= 8;
        v.tiles_per_split = (v.tile_count + v.S - 1) / v.S;
    }
    return p;
}

// The long-row search of both metrics.  c.bias == nullptr: inner product.  c.bias != nullptr: L2 over float32 rows (the
// L2 family's buffers are checked first, as sss_l2_topk_long always has) -- k_scan_long<DT_F16, 1> seeds every accumulator
// from its row's bias and norm, the ThrArgs carry metric 1, and everything else -- the level plan, launch_bound_prepare,
// launch_select_all -- is what the inner product runs.  Two things differ (select_thr.hip: THE PER-ROW BOUND): the sample
// levels scan keys LOWERED by each row's own error bound and the last level keys RAISED by it, and the levels are never
// disjoint.  All checks come before the first launch.
static int topk_long_impl(const SearchCall& c) {
    int rc = c.family == FAM_L2 ? check_buffers(c, true, false) : SSS_OK;
    if (rc) return rc;
    const bool l2 = c.bias != nullptr;
    if (c.nq <= 0 || c.n <= 0 || c.k <= 0) { set_error("%s: nq, n, k must be positive", c.what); return SSS_EINVAL; }
    rc = check_scan_source(c, true);
    if (rc) return rc;
    if (c.k > LONG_MAX_K) { set_error("%s: k too large (max %d)", c.what, LONG_MAX_K); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(c.ws) & 255) { set_error("%s: workspace must be 256-byte aligned", c.what); return SSS_EINVAL; }
    const LongLayout l = long_layout(c.nq, c.d, l2);
    if (c.ws_bytes < l.total) { set_error("%s: workspace %zu < %zu", c.what, c.ws_bytes, l.total); return SSS_EWORKSPACE; }
    char* w = reinterpret_cast<char*>(c.ws);
    void* qimg = w + l.qimg;
    int* qsel = reinterpret_cast<int*>(w + l.qsel);
    float* seed = l2 ? reinterpret_cast<float*>(w + l.seed) : nullptr;

    // the scaled image and stored f16 rows share k_scan_long<DT_F16>
    void (*kernel)(const LongArgs) = l2 ? k_scan_long<DT_F16, 1> : c.scan_dtype != DT_BF16 ? k_scan_long<DT_F16> : k_scan_long<DT_BF16>;
    const size_t lds = LT_LDS_BYTES;
    rc = opt_in_lds(reinterpret_cast<const void*>(kernel), "k_scan_long", lds);
    if (rc) return rc;
    // the f16 query image, the identity selection, D_out at "no bound known", thresholds, counters, status and the
    // per-query bound cache are written by ONE launch
    const int cap = long_cap(c.d, c.exact_dtype);
    ThrArgs t = thr_args(c, cap);
    t.qsel = qsel;
    t.thr = reinterpret_cast<float*>(w + l.thr);
    t.cnt = reinterpret_cast<unsigned*>(w + l.cnt);
    t.cand = reinterpret_cast<unsigned long long*>(w + l.cand);
    t.qb = reinterpret_cast<double*>(w + l.qb);
    rc = launch_long_setup(t, qsel, c.scan_dtype == DT_F16 ? qimg : nullptr, seed, c.st);
    if (rc) return rc;
    t.qb_ready = 1;
    LongArgs a;
    a.Qimg = c.scan_dtype == DT_F16 ? qimg : c.q;
    a.C = c.c_scan; a.nq = (int)c.nq; a.n = (int)c.n; a.d = c.d; a.G = (int)((c.nq + LT_Q - 1) / LT_Q);
    a.cap = cap; a.thr = t.thr; a.cnt = t.cnt; a.cand = const_cast<unsigned long long*>(t.cand);
    a.bias = c.bias;
    a.gpx = a.G;                    // groups per XCD (block map of k_scan_long): all of them (fewer measured slower, see the kernel)
    const LongPlan plan = long_plan((int)((c.n + LT_ROWS - 1) / LT_ROWS), cap, c.k, l2, a.G);
    for (int i = 0; i < plan.levels; ++i) {
        const LongLevel& v = plan.level[i];
        const bool last = i == plan.levels - 1;
        a.tile_count = v.tile_count; a.total_tiles = v.total_tiles; a.skip_R = v.skip_R; a.dense = v.dense;
        a.S = v.S; a.tiles_per_split = v.tiles_per_split;
        a.seed = l2 ? seed + (last ? 2 * c.nq : 0) : nullptr;
        // (thresholds and counters of this level: written by launch_long_setup -- first level -- or by the previous level's
        //  launch_bound_prepare)
        hipLaunchKernelGGL(kernel, dim3(a.S * a.G), dim3(LT_THREADS), lds, c.st, a);
        rc = check_launch("k_scan_long");
        if (rc) return rc;
        if (last) rc = launch_select_all(t, c.st);
        else {
            t.keep = v.keep;        // bound from this level's kept scan scores -> the next level's thresholds
            rc = launch_bound_prepare(t, c.st);
        }
        if (rc) return rc;
    }
    return SSS_OK;
}

extern "C" int sss_ip_topk_long(const void* q, int64_t nq, const void* corpus, int dtype, const void* scan_image, int corpus_shift,
                                float corpus_resid_norm, int64_t n, int d, int k, int64_t id_offset, float corpus_max_norm,
                                float* D_out, int64_t* I_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_long_impl({.what = "ip_topk_long", .family = FAM_IP, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = dtype, .c_scan = scan_image,
                           .scan_dtype = long_scan_dtype(dtype), .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .n = n, .d = d, .k = k,
                           .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status, .ws = workspace,
                           .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

// L2 top-k of long float32 rows (include/sss_l2_long.h)
extern "C" int sss_l2_topk_long(const float* q, int64_t nq, const float* corpus, const void* scan_image, int corpus_shift,
                                float corpus_resid_norm, const float* bias, int64_t n, int d, int k, int64_t id_offset,
                                float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, void* workspace,
                                size_t workspace_bytes, void* stream) {
    return topk_long_impl({.what = "l2_topk_long", .family = FAM_L2, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = DT_F32, .c_scan = scan_image,
                           .scan_dtype = DT_F16, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .bias = bias, .n = n, .d = d, .k = k,
                           .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status, .ws = workspace,
                           .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

}  // namespace sss
