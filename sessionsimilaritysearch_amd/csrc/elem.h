// Element formats in ONE place: the type codes, what the device needs to read a stored element (Elem<DT>), what the
// host needs to know about a format (FORMATS) and the step from a runtime code to a compile-time one (with_dtype).
// Adding a storage format: DESIGN.md "adding a storage format".  gfx950 only.
#pragma once
#include <string>
#include <type_traits>
#include "sss_common.h"

namespace sss {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int DT_F32 = 0;       // element type codes of the C ABI (include/sss.h: dtype)
constexpr int DT_BF16 = 1;
// Scan-only element type (never crosses the C ABI as a corpus dtype): an f32 corpus row of d
// elements stored as [hi(d) | lo(d)] bfloat16, hi = rne_bf16(x), lo = rne_bf16(x - hi) -- 4 bytes
// per element like f32.  The scan scores hi*hi + hi*lo + lo*hi on the bf16 MFMA (three passes at
// 16x the f32 MFMA rate); queries are f32 and are split by the kernel.  Candidates are re-scored
// from the f32 rows, and the proof uses the split's own error bound (select_dev.h: err_bound).
constexpr int DT_SPLIT = 2;
// Scan-only element type: an f32 corpus stored as float16 after an exact power-of-two scaling,
// x * 2^shift with ONE shift for the whole corpus chosen so that the largest |element| lies in
// [2^12, 2^13) (f16_shift below: far from both ends of the f16 range) -- 2 bytes per element.  The
// kernel scales each f32 query by its own power of two the same way, so a scan score is the true
// score times 2^(corpus shift + query shift): thresholds and candidate selection work in that
// domain (per query it is a fixed positive factor), and the select kernel divides it out for the
// proof.  One f16 MFMA pass (1/3 of DT_SPLIT's matrix work, half its bytes) with a coarser bound
// (select_dev.h: err_bound ~ 2^-10 |q||c|), still proven per query and re-scored from the f32 rows.
constexpr int DT_F16 = 3;
// Corpus dtype of the C ABI (include/sss.h: dtype 4) and its own scan type: rows STORED as IEEE float16 (round to
// nearest even of whatever the caller had), queries float16 too.  Rows and queries go into v_mfma_f32_32x32x16_f16 as
// they are -- no scaling, no residual, scan scores are scores -- and the candidates are re-scored from the same rows.
// (3 stays the scaled image of an f32 corpus: the two share the MFMA and the operand layout, not the bound.)
constexpr int DT_H16 = 4;
// Corpus dtype of the C ABI (include/sss.h: dtype 6; 5 stays unassigned) and its own scan type: rows STORED as int8,
// queries int8 too, 1 byte per element.  Rows and queries go into v_mfma_i32_32x32x32_i8 as they are, 16 elements per
// 16-byte chunk; products and sums are exact in int32, and for the fused shapes (d <= 1024) |score| <= d * 2^14 <= 2^24
// is exact in float32 as well: the scan score IS the canonical score (select_dev.h: err_bound = 0).
constexpr int DT_I8 = 6;

// ---- device: a STORED element type (what crosses the C ABI as a corpus dtype).  A row is read in 16-byte chunks of
// per_chunk elements; every conversion to float32 / float64 below is exact.
//   to_f32(row, i)       element i of a row in memory (16-bit formats: from_bits of its bit pattern)
//   from_word(w, j)      element j of the 32-bit word w of a row (a query row read through the scalar cache; a chunk
//                        already in registers)
//   chunk_sumsq(ss, v)   ss += the chunk's squares (sum_t: the row norm kernels' accumulator)
template <int DT>
struct Elem;

// 16-bit float formats: a word's two squares are added to each other, then to the sum
template <class E>
__device__ __forceinline__ double pair_chunk_sumsq(double ss, u32x4 v) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const double lo = E::from_word(v[w], 0), hi = E::from_word(v[w], 1);
        ss += lo * lo + hi * hi;
    }
    return ss;
}

template <>
struct Elem<DT_F32> {
    static constexpr int bytes = 4, per_chunk = 16 / bytes;
    typedef double sum_t;
    static __device__ __forceinline__ float to_f32(const void* row, int i) { return reinterpret_cast<const float*>(row)[i]; }
    static __device__ __forceinline__ float from_word(unsigned w, int) { return __builtin_bit_cast(float, w); }
    static __device__ __forceinline__ double chunk_sumsq(double ss, u32x4 u) {
        const f32x4 v = __builtin_bit_cast(f32x4, u);
        return ss + ((double)v.x * v.x + (double)v.y * v.y + (double)v.z * v.z + (double)v.w * v.w);
    }
};

template <>
struct Elem<DT_BF16> {
    static constexpr int bytes = 2, per_chunk = 16 / bytes;
    typedef double sum_t;
    static __device__ __forceinline__ float from_bits(unsigned short b) { return __builtin_bit_cast(float, (unsigned)b << 16); }
    static __device__ __forceinline__ float to_f32(const void* row, int i) { return from_bits(reinterpret_cast<const unsigned short*>(row)[i]); }
    static __device__ __forceinline__ float from_word(unsigned w, int j) { return __builtin_bit_cast(float, (j & 1) ? (w & 0xFFFF0000u) : (w << 16)); }
    static __device__ __forceinline__ double chunk_sumsq(double ss, u32x4 v) { return pair_chunk_sumsq<Elem>(ss, v); }
};

template <>
struct Elem<DT_H16> {
    static constexpr int bytes = 2, per_chunk = 16 / bytes;
    typedef double sum_t;
    static __device__ __forceinline__ float from_bits(unsigned short b) { return (float)__builtin_bit_cast(_Float16, b); }
    static __device__ __forceinline__ float to_f32(const void* row, int i) { return from_bits(reinterpret_cast<const unsigned short*>(row)[i]); }
    static __device__ __forceinline__ float from_word(unsigned w, int j) { return from_bits((unsigned short)((j & 1) ? w >> 16 : w & 0xFFFFu)); }
    static __device__ __forceinline__ double chunk_sumsq(double ss, u32x4 v) { return pair_chunk_sumsq<Elem>(ss, v); }
};

template <>
struct Elem<DT_I8> {
    static constexpr int bytes = 1, per_chunk = 16 / bytes;
    typedef long sum_t;                              // a row's sum of squares is an integer: exact in int64
    static __device__ __forceinline__ float to_f32(const void* row, int i) { return (float)reinterpret_cast<const signed char*>(row)[i]; }
    static __device__ __forceinline__ float from_word(unsigned w, int j) { return (float)(signed char)(w >> (8 * j)); }
    static __device__ __forceinline__ long chunk_sumsq(long ss, u32x4 v) {
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
            for (int b = 0; b < 4; ++b) { const int t = (int)(signed char)(v[w] >> (8 * b)); ss += t * t; }
        return ss;
    }
};

// ---- host: every format a kernel reads.  corpus: crosses the C ABI as a corpus `dtype` (else a scan-only image of an
// f32 corpus); name: what the "scan image missing" message calls it, its first word what row_align_text calls it.
struct Format { int code; int bytes; bool corpus; const char* name; };
constexpr Format FORMATS[] = {
    {DT_F32, Elem<DT_F32>::bytes, true, "f32 corpus"},   {DT_BF16, Elem<DT_BF16>::bytes, true, "bf16 corpus"},
    {DT_SPLIT, 4, false, "split image"},                 {DT_F16, 2, false, "f16 image"},
    {DT_H16, Elem<DT_H16>::bytes, true, "f16 corpus"},   {DT_I8, Elem<DT_I8>::bytes, true, "int8 corpus"},
};
static inline const Format* format_of(int dtype) {
    for (const Format& f : FORMATS)
        if (f.code == dtype) return &f;
    return nullptr;
}
static inline int elem_bytes(int dtype) { const Format* f = format_of(dtype); return f ? f->bytes : 4; }
static inline int elems_per_chunk(int dtype) { return 16 / elem_bytes(dtype); }   // a stored row is read in 16-byte pieces: d % this == 0
static inline bool corpus_dtype_ok(int dtype) { const Format* f = format_of(dtype); return f && f->corpus; }   // what crosses the C ABI as `dtype`

// "d % 4 == 0 (f32) / d % 8 == 0 (bf16, f16) / d % 16 == 0 (int8)": the row alignment of every corpus format, for
// the messages that spell it out (as a %s argument of set_error).
static inline const char* row_align_text() {
    static const std::string text = [] {
        std::string s;
        for (int per = 1; per <= 16; per <<= 1) {
            std::string names;
            for (const Format& f : FORMATS)
                if (f.corpus && 16 / f.bytes == per) names += (names.empty() ? "" : ", ") + std::string(f.name, std::string(f.name).find(' '));
            if (!names.empty()) s += (s.empty() ? "" : " / ") + ("d % " + std::to_string(per) + " == 0 (" + names + ")");
        }
        return s;
    }();
    return text.c_str();
}

// What scans rows of exact_dtype: f32 rows themselves or one of their scan-only images (long rows: the f16 image
// only); bf16, f16 and int8 rows themselves -- and int8 rows have no long-row scan.
static inline bool scan_pair_ok(int exact_dtype, int scan_dtype, bool long_rows) {
    if (!corpus_dtype_ok(exact_dtype) || !format_of(scan_dtype)) return false;
    if (exact_dtype != DT_F32) return scan_dtype == exact_dtype && !(long_rows && exact_dtype == DT_I8);
    return long_rows ? scan_dtype == DT_F16 : (scan_dtype == DT_F32 || !corpus_dtype_ok(scan_dtype));
}

// f(std::integral_constant<int, DT>) for the runtime code `dtype`: a stored type, or -- IMAGES -- a scan-only image
// as well.  False, and f not called, for any other code.
template <bool IMAGES = false, class F>
static inline bool with_dtype(int dtype, F&& f) {
    switch (dtype) {
        case DT_F32: f(std::integral_constant<int, DT_F32>()); return true;
        case DT_BF16: f(std::integral_constant<int, DT_BF16>()); return true;
        case DT_H16: f(std::integral_constant<int, DT_H16>()); return true;
        case DT_I8: f(std::integral_constant<int, DT_I8>()); return true;
        case DT_SPLIT: if constexpr (IMAGES) { f(std::integral_constant<int, DT_SPLIT>()); return true; } return false;
        case DT_F16: if constexpr (IMAGES) { f(std::integral_constant<int, DT_F16>()); return true; } return false;
    }
    return false;
}

}  // namespace sss
