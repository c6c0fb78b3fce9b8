// Device helpers of the scan kernel (scan.hip: k_scan and its threshold form).  gfx950 only.
#pragma once
#include "scan.h"

namespace sss {

typedef char __attribute__((address_space(3)))* lptr_c;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef int i32x4 __attribute__((ext_vector_type(4)));       // 16 int8 values: one A / B operand of v_mfma_i32_32x32x32_i8
typedef int i32x16 __attribute__((ext_vector_type(16)));     // its int32 accumulators (the C / D layout of the 16-bit forms)

// Sorted (descending) insert of (x, id) into a register list; lanes whose x does not beat
// their list tail fall through untouched.
template <int N>
__device__ __forceinline__ void list_insert(float (&ls)[N], int (&li)[N], float x, int id) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool c = x > ls[i];
        const float ns = c ? x : ls[i];
        const int ni = c ? id : li[i];
        x = c ? ls[i] : x;
        id = c ? li[i] : id;
        ls[i] = ns;
        li[i] = ni;
    }
}

__device__ __forceinline__ float vmax3(float a, float b, float c) {
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// The same right behind the 16-pass MFMA that wrote a, b or c: its 19 wait states first, inside the statement -- hipcc pads
// the distance from an MFMA to its own instructions, not to the inside of an asm statement.
__device__ __forceinline__ float vmax3_settled(float a, float b, float c) {
    float r;
    asm volatile("s_nop 15\n\ts_nop 2\n\tv_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Maximum of elements 0 .. 14 of an accumulator, a chain of seven v_max3 (element 15 goes into the v_max3 the caller
// finishes with).  SETTLED: the chain starts right behind the MFMA that wrote `a`.
template <bool SETTLED = false>
__device__ __forceinline__ float acc_max15(const f32x16& a) {
    float m = SETTLED ? vmax3_settled(a[0], a[1], a[2]) : vmax3(a[0], a[1], a[2]);
#pragma unroll
    for (int j = 3; j < 15; j += 2) m = vmax3(m, a[j], a[j + 1]);
    return m;
}
// ... of two accumulators, the chains interleaved
__device__ __forceinline__ void acc_max15(const f32x16& a0, const f32x16& a1, float& m0, float& m1) {
    m0 = vmax3(a0[0], a0[1], a0[2]); m1 = vmax3(a1[0], a1[1], a1[2]);
#pragma unroll
    for (int j = 3; j < 15; j += 2) { m0 = vmax3(m0, a0[j], a0[j + 1]); m1 = vmax3(m1, a1[j], a1[j + 1]); }
}

// Element j of a lane's 16 values of a 32x32 MFMA accumulator is row acc_row(j) + 4 * (lane >> 5) of the unit's 32
// (acc_row(j, first): counted from the row `first` of the lane's element 0).
__device__ __forceinline__ constexpr int acc_row(int j, int first = 0) { return first + (j & 3) + 8 * (j >> 2); }

// Ragged last tile: the elements of an accumulator whose corpus row lies at or beyond n become -inf (`first`: the corpus
// row of the lane's element 0).  (n and, below, bias_of's sub-step by reference: the callers are lambdas that reach them
// through their captures, and with a by-value copy hipcc compiles the f32 step-order kernels differently.)
__device__ __forceinline__ void mask_rows(f32x16& a, int first, const int& n) {
#pragma unroll
    for (int j = 0; j < 16; ++j)
        if (acc_row(j, first) >= n) a[j] = -INFINITY;
}
// ... of the two accumulators of a step, a1's rows 32 further
__device__ __forceinline__ void mask_rows(f32x16& a0, f32x16& a1, int first, const int& n) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int rr = acc_row(j, first);
        if (rr >= n) a0[j] = -INFINITY;
        if (rr + 32 >= n) a1[j] = -INFINITY;
    }
}

// One LDS-DMA wave-instruction: 64 lanes x 16 bytes from `base` (wave-uniform: an SGPR pair) + the lane's byte offset to
// the 1 KiB of LDS at the wave-uniform address lds_dst, lane-linear.  SC1: agent scope (not served from this CU's L1).
// (Inline asm, so hipcc neither counts it nor drains vmcnt(0) at the next ds_read.  M0 is written without a save /
//  restore: hipcc has no use of its own for M0 in the scan kernels -- no dynamic register indexing, no LDS-direct / GWS /
//  sendmsg; every M0 reference in their ISA comes from this statement.)
template <bool SC1 = false, class Base>
__device__ __forceinline__ void lds_dma16(unsigned lane_off, unsigned lds_dst, Base base) {
    if constexpr (SC1)
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2 sc1" : : "v"(lane_off), "s"(lds_dst), "s"(base) : "memory");
    else
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %2" : : "v"(lane_off), "s"(lds_dst), "s"(base) : "memory");
}

// One k-group of the f32 scans: the 16-byte chunk of a row of each accumulator's 32 (a0, a1) against the query's (q) --
// eight v_mfma_f32_32x32x2_f32, the two accumulators' chains interleaved, each in the k order x, y, z, w.
__device__ __forceinline__ void mfma_f32_group(f32x16& acc0, f32x16& acc1, const f32x4& a0, const f32x4& a1, const f32x4& q) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.x, q.x, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, q.x, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.y, q.y, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, q.y, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.z, q.z, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.z, q.z, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.w, q.w, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.w, q.w, acc1, 0, 0, 0);
}
// Half of one accumulator's share of a k-group: two of its four MFMAs, where a step issues the halves apart.
__device__ __forceinline__ void mfma_f32_pair(f32x16& acc, float a_lo, float a_hi, float q_lo, float q_hi) {
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_lo, q_lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a_hi, q_hi, acc, 0, 0, 0);
}

// L2 scans: the bias of accumulator k (0, 1) in sub-step `sub` of the current tile, bcur[2 sub + k], by a select chain over
// the H compile-time sub-steps (a runtime index would send bcur to scratch).
template <int H, int N>
__device__ __forceinline__ float bias_of(const float (&bcur)[N], const int& sub, int k) {
    float b = bcur[k];
#pragma unroll
    for (int s = 1; s < H; ++s) b = sub == s ? bcur[2 * s + k] : b;
    return b;
}

// Two 16-byte agent-scope (sc1: not served from this CU's L1) loads + their wait, as ONE asm
// statement so the destinations are never touched before the data has landed.
__device__ __forceinline__ unsigned min8_sc1(const unsigned* p) {
    u32x4 a, b;
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\t"
                 "global_load_dwordx4 %1, %2, off offset:16 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b) : "v"(p) : "memory");
    const unsigned m0 = min(min(a.x, a.y), min(a.z, a.w));
    const unsigned m1 = min(min(b.x, b.y), min(b.z, b.w));
    return min(m0, m1);
}

// Compare-exchange of two u32 (ascending).
__device__ __forceinline__ void cx_u32(unsigned& a, unsigned& b) {
    const unsigned lo = min(a, b), hi = max(a, b);
    a = lo; b = hi;
}

// RANK-SELECTED THRESHOLD (cert == 1, 16 slots = 16 class maxima of one query).  Any word v that at least K2 of the
// 16 slots reach is a valid threshold (K2 distinct rows, one per class, score at least v); the old rule, "min over K2
// classes", sits near the ~37th best row seen for K2 = 12, the K2-th largest of 16 class maxima near the ~21st
// (coupon-collector ranks 12 H12 vs 16 (H16 - H4)): 1.8x fewer rows pass.  The (h = 0, 1) lane pair of a query holds
// 8 words each; with skip = 16 - K2 words allowed below the threshold, lane h takes its m_h-th smallest word,
// m_0 + m_1 = skip + 2 (m_h = skip / 2 + 1, lane 0 one more when skip is odd), and the pair's minimum is returned:
// at most m_0 - 1 + m_1 - 1 = skip words lie below it.  That is the exact (skip + 1)-th smallest when the skip words
// below it split evenly over the halves and one or two ranks lower otherwise -- for one sorting network on 8 registers,
// one cross-lane exchange and no data-dependent indexing (the exact merge of the two sorted halves cost 16 more
// registers and spilled the append form's hot loop).  A word of 0 ("class never published") sorts first: the result
// is 0 until enough classes of BOTH halves have published.  The select kernel, which runs once per query, takes the
// exact rank (select.hip: final_tau_ord) -- any threshold the scan used lies at or below it.
__device__ __forceinline__ unsigned tau_select16(unsigned (&v)[8], int skip, int h) {
    // optimal 19-comparator sorting network for 8 inputs
    cx_u32(v[0], v[1]); cx_u32(v[2], v[3]); cx_u32(v[4], v[5]); cx_u32(v[6], v[7]);
    cx_u32(v[0], v[2]); cx_u32(v[1], v[3]); cx_u32(v[4], v[6]); cx_u32(v[5], v[7]);
    cx_u32(v[1], v[2]); cx_u32(v[5], v[6]); cx_u32(v[0], v[4]); cx_u32(v[3], v[7]);
    cx_u32(v[1], v[5]); cx_u32(v[2], v[6]);
    cx_u32(v[1], v[4]); cx_u32(v[3], v[6]);
    cx_u32(v[2], v[4]); cx_u32(v[3], v[5]);
    cx_u32(v[3], v[4]);
    const int m = (skip >> 1) + ((skip & 1) && h == 0 ? 1 : 0);       // 0-based index of this lane's word, <= 4 (skip <= 8)
    unsigned mine = v[0];
    mine = m >= 1 ? v[1] : mine;
    mine = m >= 2 ? v[2] : mine;
    mine = m >= 3 ? v[3] : mine;
    mine = m >= 4 ? v[4] : mine;
    return min(mine, (unsigned)__shfl_xor((int)mine, 32));
}

// The same two agent-scope loads, handing back the 8 words (rank-selected threshold).
__device__ __forceinline__ void load8_sc1(const unsigned* p, unsigned (&v)[8]) {
    u32x4 a, b;
    asm volatile("global_load_dwordx4 %0, %2, off sc1\n\t"
                 "global_load_dwordx4 %1, %2, off offset:16 sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(a), "=&v"(b) : "v"(p) : "memory");
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// Resident queries of one 32-query MFMA B operand: lane (r, h) ends up with the 16-byte chunks of query row
// q_ld it meets in the k-groups (qc[u]: k = 16u + 8h .. + 7 for the 16-bit types, k = 32u + 16h .. + 15 for int8, chunk
// 2u + h for f32; q_shift: where a DT_F16 scan leaves the query's shift).  DT_SPLIT / DT_F16 take float32 queries and split / scale + round them here (scan.h); the others
// (DT_H16: float16 queries against float16 rows, DT_I8: int8 against int8) load the row as it is stored.
template <int RB, int DT>
__device__ __forceinline__ void load_queries(const char* __restrict__ Qb, int q_ld, int h, f32x4 (&qc)[RB / 32], int* q_shift = nullptr) {
    constexpr int NU = RB / 32;
    if constexpr (DT == DT_SPLIT) {
        // f32 queries, split here: qc[u] = hi and qc[u + NU/2] = lo of k-slice u (k = 16u + 8h .. + 7),
        // the B operands that meet chunk 2u + h of the hi half / of the lo half of a corpus row.
        const f32x4* qp = reinterpret_cast<const f32x4*>(Qb + (size_t)q_ld * RB) + 2 * h;
#pragma unroll
        for (int u = 0; u < NU / 2; ++u) {
            const f32x4 a = qp[4 * u], b = qp[4 * u + 1];
            const float x[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            bf16x8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                hi[e] = (__bf16)x[e];
                const float rem = x[e] - (float)hi[e];
                lo[e] = (__bf16)(__builtin_isfinite(rem) ? rem : 0.f);
            }
            qc[u] = __builtin_bit_cast(f32x4, hi);
            qc[u + NU / 2] = __builtin_bit_cast(f32x4, lo);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) asm volatile("" : "+v"(qc[u]));
    } else if constexpr (DT == DT_F16) {
        // f32 queries (4 * (RB / 2) bytes per row), scaled by the query's own power of two (scan.h:
        // f16_shift of its largest |element|) and rounded to f16: qc[u] = k-slice u (k = 16u + 8h .. + 7).
        const f32x4* qp = reinterpret_cast<const f32x4*>(Qb + (size_t)q_ld * (2 * RB)) + 2 * h;
        f32x4 raw[2 * NU];
        float amax = 0.f;
#pragma unroll
        for (int u = 0; u < NU; ++u) { raw[2 * u] = qp[4 * u]; raw[2 * u + 1] = qp[4 * u + 1]; }
#pragma unroll
        for (int u = 0; u < 2 * NU; ++u)
            amax = fmaxf(fmaxf(amax, fmaxf(fabsf(raw[u].x), fabsf(raw[u].y))), fmaxf(fabsf(raw[u].z), fabsf(raw[u].w)));
        amax = fmaxf(amax, __shfl_xor(amax, 32));            // the other half of the row
        const int sh = f16_shift(amax);
        if (q_shift) *q_shift = sh;                          // (the L2 scan scales its row bias by it)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const f32x4 a = raw[2 * u], b = raw[2 * u + 1];
            f16x8 v;
            v[0] = (_Float16)ldexpf(a.x, sh); v[1] = (_Float16)ldexpf(a.y, sh);
            v[2] = (_Float16)ldexpf(a.z, sh); v[3] = (_Float16)ldexpf(a.w, sh);
            v[4] = (_Float16)ldexpf(b.x, sh); v[5] = (_Float16)ldexpf(b.y, sh);
            v[6] = (_Float16)ldexpf(b.z, sh); v[7] = (_Float16)ldexpf(b.w, sh);
            qc[u] = __builtin_bit_cast(f32x4, v);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) asm volatile("" : "+v"(qc[u]));
    } else {
        const f32x4* qp = reinterpret_cast<const f32x4*>(Qb + (size_t)q_ld * RB) + h;
#pragma unroll
        for (int u = 0; u < NU; ++u) qc[u] = qp[2 * u];
        // retire the query loads HERE: otherwise hipcc sinks their counted vmcnt waits into the
        // tile loop, where they would also wait on the (uncounted) LDS-DMA of the next tile.
#pragma unroll
        for (int u = 0; u < NU; ++u) asm volatile("" : "+v"(qc[u]));
    }

}

}  // namespace sss
