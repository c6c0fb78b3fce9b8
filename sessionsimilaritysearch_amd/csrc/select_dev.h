// Device helpers shared by the select kernels -- select.hip (the fused search's select) and select_thr.hip (the threshold
// form: rung, long rows, range search): wave primitives, the canonical float64 re-score, the scan's error bound
// (err_bound), the proof window and the per-query bound every proof of exactness rests on, radix selection and sort.
#pragma once
#include "block_select.h"
#include "scan.h"

namespace sss {

constexpr int SORT_THREADS = 256;
constexpr int SA_BYTES = 128;      // rescore_kept: bytes of every row staged through LDS per step
// Re-score "element type" of the L2 metric: float32 rows and queries, the canonical chain of squared differences
// (scan.h: l2_chain_step), the score its NEGATION -- float negation is exact and commutes with the rounding to float32,
// so "(score desc, id asc)", the u64 keys and the padding serve "(distance asc, id asc)" as they are; D is negated on
// the way out (out_score).  Never a storage format: rescore_type() makes it from (dtype, metric).
constexpr int DT_F32_L2 = 100;
__device__ __forceinline__ int rescore_type(int dtype, int metric) { return metric ? DT_F32_L2 : dtype; }
__device__ __forceinline__ float out_score(float s, int metric) { return metric ? -s : s; }

// Wave-wide maximum of a u32 on the DPP network (no LDS round trips): row_shr 1/2/4/8 leave each
// 16-lane row's maximum in its last lane, row_bcast15 / row_bcast31 carry it across rows, lane 63
// holds the result.  bound_ctrl = true feeds 0 (the identity of umax) to lanes without a source.
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true));   // row_shr:1
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true));   // row_shr:2
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true));   // row_shr:4
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true));   // row_shr:8
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true));   // row_bcast:15 -> rows 1, 3
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true));   // row_bcast:31 -> rows 2, 3
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// 64-bit keys: maximum of the high words, then of the low words among the lanes that hold it.
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
    const unsigned hi = (unsigned)(v >> 32), lo = (unsigned)v;
    const unsigned mh = wave_max_u32(hi);
    const unsigned long long own = __builtin_amdgcn_ballot_w64(hi == mh);
    unsigned ml;
    if ((own & (own - 1)) == 0)                      // one lane holds the best score (the usual case): its low word
        ml = (unsigned)__builtin_amdgcn_readlane((int)lo, __builtin_ctzll(own));
    else
        ml = wave_max_u32(hi == mh ? lo : 0u);
    return ((unsigned long long)mh << 32) | ml;
}

// Cross-lane hand-off through LDS inside ONE wave: the hardware runs a wave's LDS instructions in
// order; this only stops the compiler from moving memory operations across the point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Canonical float64 score of candidate rows, FOUR lanes per row: part p of a row's 16-byte chunks is
// loaded by lane 4c + p (every load of the row in flight at once: one memory round trip instead of
// four), and the strictly sequential float64 chain runs part after part, handed from lane to lane --
// the same additions in the same order as one lane walking the row.  Candidates [c0, c0 + 16) of `sel`.
__device__ __forceinline__ double dot_chunk(double acc, const char* qrow, int v, f32x4 c, int dtype);
// (DT: the element type as a compile-time constant -- with the three-way choice inside the unrolled chain the 32 chunk
//  registers of a part went to scratch)
// UNEVEN: rows whose chunk count is no multiple of four (rb % 64 != 0: float32 rows narrower than their scan, include/sss_pad.h) --
// ceil(nchunks / 4) chunks a part, the last part short or empty (5/5/5/2 at d = 68, 1/0/0/0 at d = 4), still at most 32 a
// part.  Every lane still loads a full window of `per` chunks at constant offsets from one address -- no load is guarded by
// where the row ends (rescore_row says why) -- the window of a short or empty part CLAMPED back into the row, [nchunks - per,
// nchunks); the chain then skips the window's first chunks, which belong to the parts before.  The even form is what it
// always was: a compile-time choice, not a branch in it.
template <int DT, bool UNEVEN = false>
__device__ __forceinline__ void rescore16_t(const unsigned long long* sel, double* resc, int c0, int c1, const void* C, int rb,
                                            const char* qrow, int lane) {
    constexpr int dtype = DT;
    const int c = c0 + (lane >> 2), p = lane & 3;
    const int nch = rb / 16;
    const int per = UNEVEN ? (nch + 3) / 4 : rb / 64;              // chunks per part: 4 / 8 / 16 / 32 (rows of 256 .. 2048 bytes)
    const unsigned long long key = c < c1 ? sel[c] : 0ull;
    const bool live = key != 0 && key_id(key) >= 0;
    constexpr int MAXP = 32;
    f32x4 ch[MAXP];
    const int first = UNEVEN ? min(p * per, nch - per) : p * per;  // the lane's window: chunks [first, first + per)  (per <= nch)
    const char* row = reinterpret_cast<const char*>(C) + (size_t)(live ? key_id(key) : 0) * rb + (size_t)first * 16;
#pragma unroll
    for (int i = 0; i < MAXP; ++i)
        if (live && i < per) ch[i] = *reinterpret_cast<const f32x4*>(row + i * 16);
    double acc = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int from = UNEVEN ? min(s * per, nch - per) : s * per;   // part s's window, and how much of it the parts before own
        const int skip = s * per - from;
        if (live && p == s) {
#pragma unroll
            for (int i = 0; i < MAXP; ++i)
                if (i < per && (!UNEVEN || i >= skip)) acc = dot_chunk(acc, qrow, from + i, ch[i], dtype);
        }
        if (s < 3) {                                               // hand the chain to the next part's lane
            const double up = __shfl_up(acc, 1);
            if (p == s + 1) acc = up;
        }
    }
    if (c < c1 && p == 3) resc[c] = live ? (DT == DT_F32_L2 ? -acc : acc) : 0.0;
}
// rb: bytes of a STORED row (stored_row_bytes); qrow holds at least as many
__device__ __forceinline__ void rescore16(const unsigned long long* sel, double* resc, int c0, int c1, const void* C, int rb,
                                          const char* qrow, int dtype, int lane) {
    if (rb & 63) {                                                 // float32 rows only (the other formats' scans take whole 256 bytes)
        if (dtype == DT_F32_L2) rescore16_t<DT_F32_L2, true>(sel, resc, c0, c1, C, rb, qrow, lane);
        else rescore16_t<DT_F32, true>(sel, resc, c0, c1, C, rb, qrow, lane);
    }
    else if (dtype == DT_F32) rescore16_t<DT_F32>(sel, resc, c0, c1, C, rb, qrow, lane);
    else if (dtype == DT_F32_L2) rescore16_t<DT_F32_L2>(sel, resc, c0, c1, C, rb, qrow, lane);
    else if (dtype == DT_H16) rescore16_t<DT_H16>(sel, resc, c0, c1, C, rb, qrow, lane);
    else if (dtype == DT_I8) rescore16_t<DT_I8>(sel, resc, c0, c1, C, rb, qrow, lane);
    else rescore16_t<DT_BF16>(sel, resc, c0, c1, C, rb, qrow, lane);
}

// the two float16 values of a 32-bit word (element 2i in the low half)
__device__ __forceinline__ _Float16 h16_lo(unsigned w) { return __builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu)); }
__device__ __forceinline__ _Float16 h16_hi(unsigned w) { return __builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }

// sum of the four int8 products of two 32-bit words (at most 4 * 2^14: exact in int32)
__device__ __forceinline__ int i8_dot4(unsigned q, unsigned c) {
    int s = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) s += (int)(signed char)(q >> (8 * b)) * (int)(signed char)(c >> (8 * b));
    return s;
}

// acc += sum over the elements of one 16-byte chunk (4 f32, 8 bf16, 8 f16 or 16 int8), sequential in k
__device__ __forceinline__ double dot_chunk(double acc, const char* qrow, int v, f32x4 c, int dtype) {
    if (dtype == DT_F32) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qrow + v * 16);
        acc += (double)qv.x * (double)c.x;
        acc += (double)qv.y * (double)c.y;
        acc += (double)qv.z * (double)c.z;
        acc += (double)qv.w * (double)c.w;
        return acc;
    }
    if (dtype == DT_F32_L2) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qrow + v * 16);
        acc = l2_chain_step(acc, (double)qv.x, (double)c.x);
        acc = l2_chain_step(acc, (double)qv.y, (double)c.y);
        acc = l2_chain_step(acc, (double)qv.z, (double)c.z);
        acc = l2_chain_step(acc, (double)qv.w, (double)c.w);
        return acc;
    }
    const u32x4 cu = __builtin_bit_cast(u32x4, c);
    const u32x4 qu = *reinterpret_cast<const u32x4*>(qrow + v * 16);
    if (dtype == DT_I8) {
        // Every product and every partial sum of the float64 chain is an integer below 2^53, so the chain rounds nowhere
        // and equals the integer sum in any order: the chunk's 16 products are summed in int32 and added once.
        acc += (double)(i8_dot4(qu.x, cu.x) + i8_dot4(qu.y, cu.y) + i8_dot4(qu.z, cu.z) + i8_dot4(qu.w, cu.w));
        return acc;
    }
    if (dtype == DT_H16) {                                        // f16 -> f64 is exact (subnormals included)
#define SSS_H2(w)                                                                                     \
    acc += (double)h16_lo(qu.w) * (double)h16_lo(cu.w);                                               \
    acc += (double)h16_hi(qu.w) * (double)h16_hi(cu.w);
        SSS_H2(x) SSS_H2(y) SSS_H2(z) SSS_H2(w)
#undef SSS_H2
        return acc;
    }
#define SSS_BF2(w)                                                                                              \
    acc += (double)__builtin_bit_cast(float, qu.w << 16) * (double)__builtin_bit_cast(float, cu.w << 16);      \
    acc += (double)__builtin_bit_cast(float, qu.w & 0xFFFF0000u) * (double)__builtin_bit_cast(float, cu.w & 0xFFFF0000u);
    SSS_BF2(x) SSS_BF2(y) SSS_BF2(z) SSS_BF2(w)
#undef SSS_BF2
    return acc;
}

// Canonical float64 score of ONE stored row by one thread: the row's 16-byte chunks are fetched sixteen at a time
// (sixteen loads in flight, one memory round trip per 256 bytes instead of one per chunk) and folded into the
// strictly sequential chain in k order.
__device__ __forceinline__ double rescore_row(const char* qrow, const char* row, int nchunks, int dtype) {
    double acc = 0.0;
    int v0 = 0;
    // full batches: sixteen UNCONDITIONAL loads (a guarded load sits in a basic block of its own and hipcc then drains
    // vmcnt before every one of them -- measured on 1600-wide rows: one load in flight, 1.4 us per 16-byte chunk)
    for (; v0 + 16 <= nchunks; v0 += 16) {
        f32x4 c[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = *reinterpret_cast<const f32x4*>(row + (size_t)(v0 + i) * 16);
#pragma unroll
        for (int i = 0; i < 16; ++i) acc = dot_chunk(acc, qrow, v0 + i, c[i], dtype);
    }
    if (v0 < nchunks) {                             // tail: the same loads clamped to the row's last chunk, their results unused
        f32x4 c[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) c[i] = *reinterpret_cast<const f32x4*>(row + (size_t)min(v0 + i, nchunks - 1) * 16);
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (v0 + i < nchunks) acc = dot_chunk(acc, qrow, v0 + i, c[i], dtype);
    }
    return dtype == DT_F32_L2 ? -acc : acc;
}

__device__ __forceinline__ float elem_to_f32(const void* row, int kk, int dtype) {
    if (dtype == DT_F32 || dtype == DT_F32_L2) return reinterpret_cast<const float*>(row)[kk];
    if (dtype == DT_I8) return (float)reinterpret_cast<const signed char*>(row)[kk];
    const unsigned short b = reinterpret_cast<const unsigned short*>(row)[kk];
    if (dtype == DT_H16) return (float)__builtin_bit_cast(_Float16, b);   // f16 -> f32 is exact
    return __builtin_bit_cast(float, (unsigned)b << 16);          // bf16 -> f32 is exact
}

// B = rounding-error bound of the scan's score of any row, by what the scan computed:
//   DT_F32   k-ordered f32 fma chain:                               d * 2^-24 * |q| |c|
//   DT_BF16  exact bf16 products summed in f32 with unspecified internal order / truncation:
//                                                                  d * 2^-23 * |q| |c|
//   DT_SPLIT x = xh + xl + xr with |x - xh| <= 2^-8 |x|, |xr| <= 2^-16 |x| (two roundings to 8
//            significant bits), likewise y; the scan sums xh*yh + xh*yl + xl*yh, so per element it
//            misses xl*yl + xr*y + (xh + xl)*yr <= 3.03 * 2^-16 |x||y|, and sum |x_k||y_k| <= |q||c|;
//            the 3d exact products (sum of magnitudes <= 1.016 |q||c|) are accumulated in f32 like
//            the bf16 case:                        (3.03 * 2^-16 + 3d * 2^-23 * 1.016) * |q| |c|
//   DT_F16   corpus and query each scaled by a power of two (exact) and rounded to 11 significant
//            bits; with c^ = c + rc, q^ = q + rq the scan sums c^ . q^ = c.q + rc.q + c^.rq, so by
//            Cauchy-Schwarz the rounding costs at most Rc |q| + (|c| + Rc) Rq, where Rc = the largest
//            row residual norm |c^ - c| over the corpus (measured when the image is built, passed in;
//            worst case 2^-11 |c|) and Rq = this query's residual norm (measured here).  Elements below
//            the f16 normal range (2^-14 in the scaled domain = 2^-26 of the largest element) add at
//            most 2^-25 sqrt(d) |q||c| even if the matrix unit flushed them; products of two f16 are
//            exact in f32 and accumulate like the bf16 case:
//                         Rc |q| + (|c| + Rc) Rq + (2^-25 sqrt(d) + d * 2^-23) |q| |c|
//   DT_H16   rows and queries STORED as float16 and fed to the f16 MFMA as they are: no rounding of inputs at all.
//            A product of two f16 values has 22 significant bits and lies in [2^-48, 2^32): exact in f32, and so
//            is every partial sum's grid (multiples of 2^-48); what remains is the f32 accumulation, as for bf16:
//                                                                  d * 2^-23 * |q| |c|
//   DT_I8    rows and queries STORED as int8 and fed to the i8 MFMA as they are, int32 accumulators: products and sums
//            of integers, exact in any order.  The scan key is that int32 converted to float32, exact while
//            |score| <= d * 2^14 <= 2^24 -- the premise d <= 1024, which the fused shapes' row sizes enforce
//            (ip_topk.hip: fused_shape_ok; 1 byte per element, rows of at most 1024 bytes).  The scan score IS the
//            canonical score:                                               0
//            (what is left of the proof window is its float32 ulp term: a proof fails on exact ties at rank k and,
//             near |score| = 2^24 where that term reaches 4, on scores within 4 of the k-th)
// (each with 2 % headroom; |c| <= the corpus' largest row norm, an upper bound at any magnitude: rowops.hip).
// The relative terms assume normal float32 arithmetic.  Where the f32 values of a chain fall below FLT_MIN = 2^-126
// they lose up to half a subnormal spacing (2^-150) per rounding, or -- if a unit flushes subnormals -- the whole
// value (< 2^-126).  Absolute floor, per chain of d products and d sums (the split scan's passes are three chains):
//   DT_F32   the f32 MFMA keeps subnormals (kernel mode; ISA: C / D never flush): d * 2^-149
//   DT_BF16, DT_SPLIT  (no assumption about the bf16 unit's subnormals): 2 d * 2^-126 per chain, and an input
//            element below 2^-126 (flushed, or -- split -- a lo / hi part rounded in the bf16 subnormal range) misses
//            at most 2^-126 |y_k| per element of the other side: sqrt(d) 2^-126 (|q| + |c|) per pass
//   DT_F16   sums and products of the scaled f16 image live in [2^-48, 2^26] x d: no floor needed
//   DT_H16   products are multiples of 2^-48 below 2^32 and sums stay below d * 2^32: nothing in the chain comes near
//            FLT_MIN or FLT_MAX whatever the stored magnitudes (f16 subnormals, 65504), so no floor here either --
//            where bf16 rows, with float32's exponent range, need one.  f16 subnormal INPUTS are kept by the matrix
//            unit: its A / B operands follow the kernel's f16 denormal mode, which hipcc leaves at "keep"
//            (tests/test_f16_index_gpu.py scans a corpus of nothing but f16 subnormals)
// A proof among subnormal-range scores thus holds whatever the unit did with them; where the floor is as wide as the
// gaps between the scores the query stays unproven and is resolved exactly by the threshold rung or the exhaustive
// kernels.
__device__ __forceinline__ double err_bound(int d, int scan_dtype, double qnorm, double cmax, double c_resid, double q_resid) {
    constexpr double U126 = 1.1754943508222875e-38, U149 = 1.4012984643248171e-45;   // 2^-126, 2^-149
    const double rd = sqrt((double)d);
    double b;
    if (scan_dtype == DT_F32) b = (double)d * 5.9604644775390625e-08 * qnorm * cmax + (double)d * U149;
    else if (scan_dtype == DT_BF16) b = (double)d * 1.1920928955078125e-07 * qnorm * cmax + (2.0 * d + rd * (qnorm + cmax)) * U126;
    else if (scan_dtype == DT_H16) b = (double)d * 1.1920928955078125e-07 * qnorm * cmax;
    else if (scan_dtype == DT_I8) b = 0.0;
    else if (scan_dtype == DT_SPLIT) b = (3.03 * 1.52587890625e-05 + 3.0 * (double)d * 1.1920928955078125e-07 * 1.016) * qnorm * cmax +
                                         3.0 * (2.0 * d + rd * (qnorm + cmax)) * U126;
    else b = c_resid * qnorm + (cmax + c_resid) * q_resid +
             (2.98023223876953125e-08 * rd + (double)d * 1.1920928955078125e-07) * qnorm * cmax;
    return b * 1.02;
}

// THE L2 BOUND.  The score of the L2 metric is s = -dist, dist the canonical chain of squared differences; in real
// arithmetic s = 2 (q.c - |c|^2 / 2) - |q|^2, and the L2 scan's key of a row is kappa~ ~ sigma (q.c + b^), b^ the stored
// float32 bias and sigma = 2^(corpus shift + query shift) for the DT_F16 scan, else 1.  The score bound of a key is
//     kappa~ * (2 / sigma) - qn2  (qn2: |q|^2 summed in float64),   and  |bound - s| <= B_l2 =
//   2 x [ the inner-product bound of the scan that ran, for a chain of d + 1 terms (err_bound(d + 1, ...): its terms grow with d)
//       + A(d + 1) * cmax^2 / 2     the accumulators start from the bias, so every partial sum of the chain is bounded by
//                                   |q| cmax + cmax^2 / 2 instead of |q| cmax; A is the scan's accumulation coefficient
//                                   per unit of that magnitude: d 2^-24 (DT_F32), 3 d 2^-23 (DT_SPLIT: the bias rides through
//                                   all three passes), d 2^-23 (DT_F16).  (The input roundings -- split residue, f16 residuals --
//                                   concern q.c alone: the bias is float32 in every scan, and its product with sigma is exact.)
//       + 2^-126 / sigma ]          DT_F16: a scaled bias below FLT_MIN may lose up to that much
//   + 2^-24 cmax^2                  the stored bias: -|c|^2 / 2 from a float64 sum of exact squares, rounded ONCE to float32
//                                   (2^-25 |c|^2, doubled by the factor 2 above; the float64 sum's own d 2^-53 disappears in
//                                   the headroom), and 2^-149 where it is subnormal
//   + (d + 2) 2^-53 qn2             the float64 sum of the query's exact squares, in any order
//   + (d + 3) 2^-52 (|q| + cmax)^2  the canonical chain itself against the real sum: q_k - c_k, its square and the running sum
//                                   round once each, every term and partial sum at most (|q| + cmax)^2
// with the 2 % headroom.  The subnormal floors are those of err_bound (the seed counts as one more element of the chain).
// Where B_l2 is not finite and normal -- sigma outside 2^+-120, a scaled bias that may overflow, norms beyond float32 -- it
// is +inf: the query is UNPROVEN whatever its keys are (the fused select forces the status), the rung's threshold is -inf,
// and the exhaustive kernels resolve it.  (The long-row search, whose k_select_all proves by "every kept row was
// re-scored" and forces nothing, gives such a query the threshold +inf instead -- it keeps no row: select_thr.hip,
// long_thr -- and scans with a per-row form of this bound: select_thr.hip, THE PER-ROW BOUND.)  inf - inf cannot occur in a key: the bias is finite (FlatIndex routes to the
// scan only where cmax^2 / 2 is a normal float32), so a key is finite, or q.c overflowed and it is +-inf -- ordered, never
// NaN -- and such a query's keys say nothing the proof accepts: +inf as the edge makes the window infinite.
__device__ __forceinline__ double err_bound_l2(int d, int scan_dtype, double qnorm, double cmax, double c_resid, double q_resid, double qn2,
                                               double sigma) {
    constexpr double U126 = 1.1754943508222875e-38, U149 = 1.4012984643248171e-45;
    const double d1 = (double)(d + 1), half = 0.5 * cmax * cmax;
    const double A = scan_dtype == DT_F32 ? d1 * 5.9604644775390625e-08 : scan_dtype == DT_SPLIT ? 3.0 * d1 * 1.1920928955078125e-07 : d1 * 1.1920928955078125e-07;
    const double scan = err_bound(d + 1, scan_dtype, qnorm, cmax, c_resid, q_resid) + 1.02 * (A * half + (scan_dtype == DT_F16 ? U126 / sigma : 0.0));
    const double sum = qnorm + cmax;
    const double b = 2.0 * scan + 1.02 * (5.9604644775390625e-08 * cmax * cmax + U149 + (double)(d + 2) * 1.1102230246251565e-16 * qn2 +
                                          (double)(d + 3) * 2.220446049250313e-16 * sum * sum);
    const bool ok = b == b && b < 1.0e300 && sigma > 7.5e-37 && sigma < 1.4e36 && half * sigma < 1.0e36;     // (2^-120 .. 2^120)
    return ok ? b : INFINITY;
}

// THE PROOF WINDOW.  A row whose scan score is `scan_score` has an exact score of at most scan_score * unscale + off + B
// (unscale: what a scan score must be multiplied by to be a score -- 1, 2^-(shifts) for DT_F16, twice that for L2 keys;
// off: 0, or -|q|^2 for L2 keys; B: err_bound / err_bound_l2).  window_top is the
// highest score such a row can still show against a reference score `ref` once both are rounded to float32: the row can
// neither pass `ref` nor tie with it if window_top < ref (ULP32_REL, ULP32_MIN: scan.h).
__device__ __forceinline__ double window_top(float scan_score, double unscale, double off, double B, double ref) {
    return (double)scan_score * unscale + off + B + ULP32_REL * fabs(ref) + ULP32_MIN;
}

// Its inverse: the scan threshold that a known lower bound `lb` of the query's k-th score allows: rows the scan does NOT keep have
// scan score <= thr, hence exact score <= thr * unscale + off + B < lb - ulp32(lb).  -inf when no bound is known (-FLT_MAX).
__device__ __forceinline__ float thr_from_bound(double lb, double B, double unscale, double off) {
    const double t = (lb - off - B - ULP32_REL * fabs(lb) - ULP32_MIN) / unscale;
    float thr = (float)t;                                                   // round to nearest, then step below
    if ((double)thr >= t) thr = nextafterf(thr, -INFINITY);
    if (!(lb > -3.0e38)) thr = -INFINITY;
    return thr;
}

// squared rounding residual of query element v under the DT_F16 scan's scaling + rounding (scan.hip)
__device__ __forceinline__ double f16_resid2(float v, int sh) {
    const double back = ldexp((double)(float)(_Float16)ldexpf(v, sh), -sh);     // (in float the scale-back of a tiny row would round)
    const double r = back - (double)v;
    return r * r;
}

// THE QUERY BOUND: B (err_bound of the scan that produced the candidates) and unscale (scan score -> score factor:
// 2^-(corpus shift + query shift) of a DT_F16 scan, scan.h; else 1) of the query row at `qrow` (LDS or global, `dtype`
// elements).  A: SelectArgs or ThrArgs (d, dtype, scan_dtype, corpus_shift, corpus_max_norm, corpus_resid; as the kernel
// argument itself -- passed field by field the threshold kernels' schedules moved).  Called by ONE whole wave; every
// lane returns the same values.  A.metric == 1 (L2 keys): B = err_bound_l2, unscale doubled, off = -|q|^2; else off = 0.
template <typename Args>
__device__ __forceinline__ void query_bound(const Args& A, const char* qrow, int lane, double& B, double& unscale, double& off) {
    const int d = A.d, dtype = A.dtype, scan_dtype = A.scan_dtype;
    double qn2 = 0.0;
    float q_amax = 0.f;
    for (int kk = lane; kk < d; kk += 64) {
        const float v = elem_to_f32(qrow, kk, dtype);
        qn2 += (double)v * (double)v;
        q_amax = fmaxf(q_amax, fabsf(v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                              // the norm only feeds the error BOUND: order-free
        qn2 += __shfl_xor(qn2, o);
        q_amax = fmaxf(q_amax, __shfl_xor(q_amax, o));
    }
    double rq2 = 0.0;
    if (scan_dtype == DT_F16) {
        const int sh = f16_shift(q_amax);
        for (int kk = lane; kk < d; kk += 64) rq2 += f16_resid2(elem_to_f32(qrow, kk, dtype), sh);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rq2 += __shfl_xor(rq2, o);
    }
    B = err_bound(d, scan_dtype, sqrt(qn2), (double)A.corpus_max_norm, (double)A.corpus_resid, sqrt(rq2));
    unscale = scan_dtype == DT_F16 ? ldexp(1.0, -(A.corpus_shift + f16_shift(q_amax))) : 1.0;
    off = 0.0;
    if (A.metric) {
        B = err_bound_l2(d, scan_dtype, sqrt(qn2), (double)A.corpus_max_norm, (double)A.corpus_resid, sqrt(rq2), qn2, 1.0 / unscale);
        unscale *= 2.0;
        off = -qn2;
    }
}

// The k-th largest score ordinal (high word of the keys) among keys[0 .. M), k <= M, by the whole workgroup of
// SORT_THREADS = 256 threads (block_select.h: kth_largest_of).  s_hist: RADIX_HIST_WORDS shared words; every thread
// returns the same value.
__device__ __forceinline__ unsigned kth_largest_ord(const unsigned long long* keys, int M, int k, int tid, unsigned* s_hist) {
    return kth_largest_of<SORT_THREADS>([&](int x) { return (unsigned)(keys[x] >> 32); }, M, k, tid, s_hist);
}

// The k-th largest 64-bit KEY among keys[0 .. M) (keys are unique: score ordinal << 32 | ~row id), k <= M: the k-th largest
// high word, then -- inside its tie group -- the low word that completes the count.  Exactly k keys lie at or above the
// result.  Whole workgroup; s_cnt: one shared word.
__device__ __forceinline__ unsigned long long kth_largest_key(const unsigned long long* keys, int M, int k, int tid, unsigned* s_hist,
                                                              unsigned* s_cnt) {
    const unsigned sk = kth_largest_of<SORT_THREADS>([&](int x) { return (unsigned)(keys[x] >> 32); }, M, k, tid, s_hist);
    if (tid == 0) *s_cnt = 0u;
    __syncthreads();
    unsigned gt = 0u;
    for (int x = tid; x < M; x += SORT_THREADS) gt += (unsigned)(keys[x] >> 32) > sk ? 1u : 0u;
    if (gt) atomicAdd(s_cnt, gt);
    __syncthreads();
    const int need_eq = k - (int)*s_cnt;                                // >= 1: the k-th itself has ordinal sk
    __syncthreads();
    const unsigned lowk = kth_largest_of<SORT_THREADS>([&](int x) { const unsigned long long kx = keys[x]; return (unsigned)(kx >> 32) == sk ? (unsigned)kx : 0u; },
                                         M, need_eq, tid, s_hist);
    return ((unsigned long long)sk << 32) | lowk;
}

// descending bitonic sort of keys[0 .. M2) (M2 a power of two) by the whole workgroup
__device__ __forceinline__ void sort_desc(unsigned long long* keys, int M2, int tid) { sort_keys<SORT_THREADS, true>(keys, M2, tid); }

// Canonical re-score of the kept rows surv[0 .. keep) (scan keys: only their ids are read) by a workgroup of SORT_THREADS,
// one thread per row for the strictly sequential float64 chain -- but rows of 1024 bytes and more come in through LDS:
// the workgroup fetches 128 contiguous bytes of each of a group's SA_ROWS rows per step (coalesced: eight lanes a row)
// and every thread then reads its own row's chunks from the staging tile `stage` ([SA_ROWS][SA_BYTES + 16]).  (A thread
// walking its own 6400-byte row 16 bytes at a time -- round 3's first form -- turned every load into 64 separate line
// requests per wave: 0.53 ms of a 5.7 ms search at D = 1600, K = 100.)  emit(c, valid, score, id) is called once for
// every c < K2 (K2 >= keep) by the thread that owns it; valid == c < keep.  qrow: the query row in LDS.
template <int SA_ROWS, typename Emit>
__device__ __forceinline__ void rescore_kept(const unsigned long long* surv, int keep, int K2, const void* C, int rb, int dtype,
                                             const char* qrow, char* stage, int tid, Emit emit) {
    const int nchunks = rb / 16;
    if (rb < 1024 || keep <= 0) {                                       // short rows (a few lines each): a thread per row, all 256 busy
                                                                        // (nothing kept: the tile's clamped fetches would have no row)
        for (int c = tid; c < K2; c += SORT_THREADS) {
            if (c < keep) {
                const int id = key_id(surv[c]);
                emit(c, true, rescore_row(qrow, reinterpret_cast<const char*>(C) + (size_t)id * rb, nchunks, dtype), id);
            } else {
                emit(c, false, 0.0, -1);
            }
        }
        return;
    }
    for (int c0 = 0; c0 < K2; c0 += SA_ROWS) {
        constexpr int PER = SA_ROWS * (SA_BYTES / 16) / SORT_THREADS;   // 16-byte pieces a thread fetches per step
        f32x4 pre[PER];
        auto fetch = [&](int b) __attribute__((always_inline)) {
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int idx = tid + SORT_THREADS * j, r = idx / (SA_BYTES / 16), ch = idx % (SA_BYTES / 16);
                const int cs = min(c0 + r, keep - 1), vs = min(b + ch, nchunks - 1);      // (clamped: unused copies of valid bytes)
                pre[j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(C) + (size_t)key_id(surv[cs]) * rb + (size_t)vs * 16);
            }
        };
        double acc = 0.0;
        fetch(0);
        for (int b = 0; b < nchunks; b += SA_BYTES / 16) {
            __syncthreads();                                            // the previous step's tile has been consumed
#pragma unroll
            for (int j = 0; j < PER; ++j) {
                const int idx = tid + SORT_THREADS * j, r = idx / (SA_BYTES / 16), ch = idx % (SA_BYTES / 16);
                *reinterpret_cast<f32x4*>(stage + r * (SA_BYTES + 16) + ch * 16) = pre[j];
            }
            __syncthreads();
            if (b + SA_BYTES / 16 < nchunks) fetch(b + SA_BYTES / 16);  // in flight under this step's chain
            if (tid < SA_ROWS && c0 + tid < keep) {
#pragma unroll
                for (int i = 0; i < SA_BYTES / 16; ++i)
                    if (b + i < nchunks)
                        acc = dot_chunk(acc, qrow, b + i, *reinterpret_cast<const f32x4*>(stage + tid * (SA_BYTES + 16) + i * 16), dtype);
            }
        }
        __syncthreads();                                                // (surv is read by every fetch; what emit writes aliases nothing)
        if (tid < SA_ROWS && c0 + tid < K2) {
            if (c0 + tid < keep) emit(c0 + tid, true, dtype == DT_F32_L2 ? -acc : acc, key_id(surv[c0 + tid]));
            else emit(c0 + tid, false, 0.0, -1);
        }
    }
}

// bytes of a STORED row of d elements (the exact element types: DT_F32, DT_I8, else DT_BF16 / DT_H16; the host's
// elem_bytes, elem.h, also knows the scan-only images)
__device__ __forceinline__ int row_bytes(int d, int dtype) { return d * (dtype == DT_F32 ? 4 : dtype == DT_I8 ? 1 : 2); }
// bytes of a stored row of C (A: SelectArgs or ThrArgs): d_row elements where the rows are narrower than the scan's d
// (include/sss_pad.h), else d.  The query rows of Q are always d wide.
template <typename Args>
__device__ __forceinline__ int stored_row_bytes(const Args& A) { return row_bytes(A.d_row ? A.d_row : A.d, A.dtype); }

// the query row q of Q (rb bytes) into LDS, by the NT threads t of its wave or workgroup
template <int NT>
__device__ __forceinline__ void load_query_row(char* qrow, const void* Q, int q, int rb, int t) {
    for (int i = t; i < rb / 16; i += NT)
        reinterpret_cast<f32x4*>(qrow)[i] = reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(Q) + (size_t)q * rb)[i];
}

// faiss pads missing results: (-FLT_MAX, -1) in the entries [from, k) of a query's result row
// (metric 1: distances, padded with +FLT_MAX)
__device__ __forceinline__ void pad_result(float* Dq, long* Iq, int j, int metric = 0) { Dq[j] = out_score(-3.4028234663852886e38f, metric); Iq[j] = -1; }
__device__ __forceinline__ void pad_results(float* Dq, long* Iq, int from, int k, int t, int nthreads, int metric = 0) {
    for (int j = from + t; j < k; j += nthreads) pad_result(Dq, Iq, j, metric);
}

}  // namespace sss
