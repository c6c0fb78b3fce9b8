// HBM-bound row kernels: L2-normalise, row-norm max, embedding-row gather (gfx950).
//
//   k_normalize_rows  <- `normalize` (reference util_amazon_filtered.py:28-31; the
//                        ||v||+1e-4 variant of fine_tune_ours.py:38-40 is rule 1)
//   k_gather_rows     <- NodeAsinEmbedding.forward (reference model/NodeEmbedding.py:137-138)
// Each row is owned by a group of LPR lanes that move 16 bytes per lane per access (coalesced
// 16 B x LPR segments); reductions are butterflies inside the lane group.
#include "elem.h"
#include "lane_group.h"

namespace sss {

template <int LPR>
__global__ __launch_bounds__(256) void k_normalize_rows(float* __restrict__ x, long n, int d, long ld,
                                                        float eps, int rule) {
    const int sub = threadIdx.x % LPR;
    const long rows_per_block = 256 / LPR;
    const int nv = d / 4;
    for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / LPR; row < n;
         row += (long)gridDim.x * rows_per_block) {
        float4* p = reinterpret_cast<float4*>(x + row * ld);
        float ss = 0.f;
        for (int i = sub; i < nv; i += LPR) {
            const float4 v = p[i];
            ss += v.x * v.x; ss += v.y * v.y; ss += v.z * v.z; ss += v.w * v.w;
        }
        ss = group_sum<LPR>(ss);
        const float den = rule == 0 ? sqrtf(fmaxf(ss, eps)) : sqrtf(ss) + eps;
        for (int i = sub; i < nv; i += LPR) {
            float4 v = p[i];
            v.x /= den; v.y /= den; v.z /= den; v.w /= den;
            p[i] = v;
        }
    }
}

// Largest row 2-norm, a true UPPER bound for any finite rows (it feeds every scan's error bound): the squares of
// float32 values are exact in float64 and their sum stays finite and normal far beyond where a float32 sum of squares
// under- or overflows (rows below ~1e-19 or above ~1.8e19); d <= 2^20 additions cost at most d 2^-53 relative, covered
// by the 1e-12 headroom, and the float32 result is rounded UP (inf when the norm itself exceeds FLT_MAX).
__device__ __forceinline__ float norm_up(double ss) {
    const double r = sqrt(ss) * (1.0 + 1e-12);
    float f = (float)r;
    if ((double)f < r) f = nextafterf(f, INFINITY);
    return f;
}

// One group of LPR lanes per row (float32 rows: the smallest power of two that covers d / 4 chunks; the other formats a
// whole wave), a lane folding the squares of the row's 16-byte chunks in the format's own accumulator (elem.h:
// chunk_sumsq -- the squares of the exactly converted values in float64; int8: an integer sum, exact in int64, so the
// value is the exact norm rounded up by norm_up).  float16 rows: a row holding an inf or a NaN reads as +inf, so one
// reduction also tells a caller that a conversion to float16 overflowed (FlatIndex.add).
template <int DT, int LPR>
__global__ __launch_bounds__(256) void k_row_norm_max(const void* __restrict__ x, long n, int d, float* __restrict__ out) {
    typedef Elem<DT> E;
    const int sub = threadIdx.x % LPR;
    const long rows_per_block = 256 / LPR;
    const int nv = d / E::per_chunk;
    double m = 0.0;
    for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / LPR; row < n;
         row += (long)gridDim.x * rows_per_block) {
        const u32x4* p = reinterpret_cast<const u32x4*>(reinterpret_cast<const char*>(x) + row * (long)d * E::bytes);
        typename E::sum_t ss = 0;
        [[maybe_unused]] bool bad = false;
        for (int i = sub; i < nv; i += LPR) {
            const u32x4 v = p[i];
            ss = E::chunk_sumsq(ss, v);
            if constexpr (DT == DT_H16) {
#pragma unroll
                for (int w = 0; w < 4; ++w) bad |= (v[w] & 0x7C00u) == 0x7C00u || (v[w] & 0x7C000000u) == 0x7C000000u;
            }
        }
        if constexpr (DT == DT_H16) {
            if (bad) ss = INFINITY;                     // (NaN would be dropped by fmax below)
        }
        ss = group_sum<LPR>(ss);
        m = fmax(m, (double)ss);
    }
    if constexpr (LPR < 64) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmax(m, __shfl_xor(m, o));
    }
    // non-negative floats order like their bit patterns
    if ((threadIdx.x & 63) == 0)
        atomicMax(reinterpret_cast<unsigned int*>(out), __builtin_bit_cast(unsigned int, norm_up(m)));
}

// float32 -> bfloat16, round to nearest even (plain cast: v_cvt_pk_bf16_f32, NaN stays NaN);
// 8 elements per thread, 32-byte loads / 16-byte stores.
typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void k_f32_to_bf16(const float* __restrict__ x, long n8, unsigned short* __restrict__ y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
        bf16x8_t o;
        o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
        o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
        reinterpret_cast<bf16x8_t*>(y)[i] = o;
    }
}

// f32 row [d] -> [hi(d) | lo(d)] bfloat16 (scan.h: DT_SPLIT): hi = rne(x), lo = rne(x - hi); a lo that
// is not finite (x = +-inf, or hi rounded up to inf) is stored as 0.  8 elements per thread.
__global__ __launch_bounds__(256) void k_split_bf16(const float* __restrict__ x, long n, int d8,
                                                    unsigned short* __restrict__ y) {
    const long total = n * d8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / d8;
        const int j = (int)(i - row * d8);
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
        const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
        bf16x8_t hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (__bf16)v[e];
            const float rem = v[e] - (float)hi[e];
            lo[e] = (__bf16)(__builtin_isfinite(rem) ? rem : 0.f);
        }
        bf16x8_t* out = reinterpret_cast<bf16x8_t*>(y) + row * 2 * d8;
        out[j] = hi;
        out[d8 + j] = lo;
    }
}

// max |x_i| over `count` contiguous floats -> *out (atomic max on the bit pattern of a non-negative
// float; caller zeroes).  NaNs are ignored (fmaxf), +-inf gives inf.  count % 4 == 0.
__global__ __launch_bounds__(256) void k_abs_max(const float* __restrict__ x, long n4, float* __restrict__ out) {
    float m = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(a.x), fabsf(a.y))), fmaxf(fabsf(a.z), fabsf(a.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<unsigned*>(out), __float_as_uint(m));
}

// f32 -> float16 of x * 2^shift (scan.h: DT_F16), round to nearest even; 8 elements per thread.
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
__global__ __launch_bounds__(256) void k_scale_f16(const float* __restrict__ x, long n8, int shift,
                                                   unsigned short* __restrict__ y) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
        const f32x4 a = reinterpret_cast<const f32x4*>(x)[2 * i], b = reinterpret_cast<const f32x4*>(x)[2 * i + 1];
        f16x8_t o;
        o[0] = (_Float16)ldexpf(a.x, shift); o[1] = (_Float16)ldexpf(a.y, shift);
        o[2] = (_Float16)ldexpf(a.z, shift); o[3] = (_Float16)ldexpf(a.w, shift);
        o[4] = (_Float16)ldexpf(b.x, shift); o[5] = (_Float16)ldexpf(b.y, shift);
        o[6] = (_Float16)ldexpf(b.z, shift); o[7] = (_Float16)ldexpf(b.w, shift);
        reinterpret_cast<f16x8_t*>(y)[i] = o;
    }
}

// max over rows of || y_i * 2^-shift - x_i ||_2 (y the scaled f16 image of x) -> *out, atomically
// maximised (caller zeroes): the corpus residual of the DT_F16 error bound.  One wave per row.
__global__ __launch_bounds__(256) void k_f16_resid_max(const float* __restrict__ x, const _Float16* __restrict__ y,
                                                       long n, int d, int shift, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    float m = 0.f;
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < n; row += (long)gridDim.x * 4) {
        double s = 0.0;
        for (int kk = lane; kk < d; kk += 64) {
            const double r = ldexp((double)(float)y[row * d + kk], -shift) - (double)x[row * d + kk];   // (float ldexpf would round a subnormal result)
            s += r * r;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        const float f = norm_up(s);                             // rounded up
        if (f == f) m = fmaxf(m, f);
    }
    if (lane == 0 && m > 0.f) atomicMax(reinterpret_cast<unsigned*>(out), __float_as_uint(m));
}

// ---- row-widening builders (include/sss_pad.h): float32 rows of d elements -> rows of ds >= d elements whose columns
// d .. ds-1 are exact +0, for the scans of a width the row does not have.  One thread per 16-byte chunk of the OUTPUT,
// consecutive threads along the row (coalesced stores; the loads of a row are as contiguous), grid-stride over n * chunks:
// any n.  d % 4 == 0: a 16-byte chunk of the input lies wholly inside the row or wholly in the padding.
__global__ __launch_bounds__(256) void k_pad_rows_f32(const float* __restrict__ x, long n, int d4, int ds4, float* __restrict__ y) {
    const long total = n * ds4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / ds4;
        const int j = (int)(i - row * ds4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (j < d4) v = reinterpret_cast<const f32x4*>(x)[row * d4 + j];
        reinterpret_cast<f32x4*>(y)[i] = v;
    }
}

// the eight float32 elements 8 j .. 8 j + 7 of a d-wide row (d4 = d / 4 chunks), zeros from column d on
__device__ __forceinline__ void load8_padded(const float* __restrict__ x, long row, int d4, int j, float v[8]) {
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4* p = reinterpret_cast<const f32x4*>(x) + row * d4;
    const f32x4 a = 2 * j < d4 ? p[2 * j] : zero, b = 2 * j + 1 < d4 ? p[2 * j + 1] : zero;
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// k_scale_f16 into ds-wide rows: the same x * 2^shift, rounded to nearest even; ldexpf(+0, shift) = +0
__global__ __launch_bounds__(256) void k_pad_scale_f16(const float* __restrict__ x, long n, int d4, int ds8, int shift,
                                                       unsigned short* __restrict__ y) {
    const long total = n * ds8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / ds8;
        float v[8];
        load8_padded(x, row, d4, (int)(i - row * ds8), v);
        f16x8_t o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (_Float16)ldexpf(v[e], shift);
        reinterpret_cast<f16x8_t*>(y)[i] = o;
    }
}

// k_split_bf16 into [hi(ds) | lo(ds)] rows: the same two roundings per element; +0 splits into (+0, +0)
__global__ __launch_bounds__(256) void k_pad_split_bf16(const float* __restrict__ x, long n, int d4, int ds8,
                                                        unsigned short* __restrict__ y) {
    const long total = n * ds8;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long row = i / ds8;
        const int j = (int)(i - row * ds8);
        float v[8];
        load8_padded(x, row, d4, j, v);
        bf16x8_t hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (__bf16)v[e];
            const float rem = v[e] - (float)hi[e];
            lo[e] = (__bf16)(__builtin_isfinite(rem) ? rem : 0.f);
        }
        bf16x8_t* out = reinterpret_cast<bf16x8_t*>(y) + row * 2 * ds8;
        out[j] = hi;
        out[ds8 + j] = lo;
    }
}

// k_f16_resid_max of d-wide rows x against their ds-wide image y: sixteen lanes a row, a lane taking eight elements per
// step (16 bytes of the image, 32 of the row); the image's columns from d on are +0 against nothing: no residual.
__global__ __launch_bounds__(256) void k_pad_f16_resid_max(const float* __restrict__ x, const _Float16* __restrict__ y, long n, int d4,
                                                           int ds8, int shift, float* __restrict__ out) {
    const int sub = threadIdx.x & 15;
    const int nj = (d4 + 1) / 2;                                   // 8-element groups that hold a column below d
    float m = 0.f;
    for (long row = (long)blockIdx.x * 16 + (threadIdx.x >> 4); row < n; row += (long)gridDim.x * 16) {
        double s = 0.0;
        for (int j = sub; j < nj; j += 16) {
            float v[8];
            load8_padded(x, row, d4, j, v);
            const f16x8_t h = reinterpret_cast<const f16x8_t*>(y)[row * ds8 + j];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const double r = ldexp((double)(float)h[e], -shift) - (double)v[e];
                s += r * r;
            }
        }
        s = group_sum<16>(s);
        const float f = norm_up(s);                                 // rounded up
        if (f == f) m = fmaxf(m, f);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0 && m > 0.f) atomicMax(reinterpret_cast<unsigned*>(out), __float_as_uint(m));
}

// bias[i] = -|c_i|^2 / 2 of float32 rows: what every score of row i starts from in the L2 scans (scan_kernel.h: k_scan<..., MET = 1>;
// |q - c|^2 = |q|^2 - 2 (q.c - |c|^2 / 2)).  The squares of float32 values are exact in float64; their sum (four lanes a
// row, then the four partial sums) is rounded ONCE to float32 -- the 2^-25 |c|^2 of select_dev.h: err_bound_l2, which also
// covers the float64 additions in whatever order.  One array per index, unscaled, for all three scans.
__global__ __launch_bounds__(256) void k_row_bias(const float* __restrict__ c, long n, int d, float* __restrict__ bias) {
    const int sub = threadIdx.x & 3;
    const int nv = d / 4;
    for (long row = (long)blockIdx.x * 64 + (threadIdx.x >> 2); row < n; row += (long)gridDim.x * 64) {
        const u32x4* p = reinterpret_cast<const u32x4*>(c + row * (long)d);
        double ss = 0.0;
        for (int i = sub; i < nv; i += 4) ss = Elem<DT_F32>::chunk_sumsq(ss, p[i]);
        ss = group_sum<4>(ss);
        if (sub == 0) bias[row] = (float)(-0.5 * ss);
    }
}

template <int LPR>
__global__ __launch_bounds__(256) void k_gather_rows(const float* __restrict__ table,
                                                     const long* __restrict__ ids, long n, int d,
                                                     float* __restrict__ out, long ld_out) {
    const int sub = threadIdx.x % LPR;
    const long rows_per_block = 256 / LPR;
    const int nv = d / 4;
    for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / LPR; row < n;
         row += (long)gridDim.x * rows_per_block) {
        const float4* src = reinterpret_cast<const float4*>(table + ids[row] * (long)d);
        float4* dst = reinterpret_cast<float4*>(out + row * ld_out);
        for (int i = sub; i < nv; i += LPR) dst[i] = src[i];
    }
}

// use_id_embedding=True of the reference encoder (model/model.py:288-289): embedding['product'] =
// concat(id_embedding(x), text_features) -- out[i] = [table[ids[i]] (d_id floats) | feat[i] (d_f floats) | pad zeros],
// one pass, one lane group per row.  feat == nullptr writes zeros there (query rows padded to the product width).
template <int LPR>
__global__ __launch_bounds__(256) void k_gather_concat_rows(const float* __restrict__ table, const long* __restrict__ ids,
                                                            int d_id, const float* __restrict__ feat, long ld_feat, int d_f,
                                                            int d_pad, long n, float* __restrict__ out, long ld_out) {
    const int sub = threadIdx.x % LPR;
    const long rows_per_block = 256 / LPR;
    const int nv_id = d_id / 4, nv_f = d_f / 4, nv_pad = d_pad / 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long row = (long)blockIdx.x * rows_per_block + threadIdx.x / LPR; row < n;
         row += (long)gridDim.x * rows_per_block) {
        float4* dst = reinterpret_cast<float4*>(out + row * ld_out);
        if (nv_id) {
            const float4* src = reinterpret_cast<const float4*>(table + ids[row] * (long)d_id);
            for (int i = sub; i < nv_id; i += LPR) dst[i] = src[i];
        }
        if (feat) {
            const float4* f = reinterpret_cast<const float4*>(feat + row * ld_feat);
            for (int i = sub; i < nv_f; i += LPR) dst[nv_id + i] = f[i];
        } else {
            for (int i = sub; i < nv_f; i += LPR) dst[nv_id + i] = zero;
        }
        for (int i = sub; i < nv_pad; i += LPR) dst[nv_id + nv_f + i] = zero;
    }
}

// the lane-group kernels here grid-stride over their rows: ~8 workgroups per CU
constexpr long GRID_CAP = 256 * 8;

extern "C" int sss_normalize_rows(float* x, int64_t n, int d, int64_t ld, float eps, int rule, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d <= 0 || d % 4 || ld < d || ld % 4 || (rule != 0 && rule != 1)) {
        set_error("normalize_rows: need n >= 0, d %% 4 == 0, ld >= d, ld %% 4 == 0, rule in {0,1}");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    const int lpr = lanes_for(d);
    SSS_LPR_SWITCH(lpr, hipLaunchKernelGGL(k_normalize_rows<L>, dim3(grid_blocks(n, 256 / L, GRID_CAP)), dim3(256), 0, st, x, n, d, ld, eps, rule));
    return check_launch("k_normalize_rows");
}

extern "C" int sss_row_norm_max(const void* x, int64_t n, int d, int dtype, float* out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!corpus_dtype_ok(dtype) || n < 0 || d <= 0 || d % elems_per_chunk(dtype)) {
        set_error("row_norm_max: need dtype in {0,1,4,6}, n >= 0, %s", row_align_text());
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    with_dtype(dtype, [&](auto dt) {
        constexpr int DT = decltype(dt)::value;
        if constexpr (DT == DT_F32) {
            SSS_LPR_SWITCH(lanes_for(d), hipLaunchKernelGGL((k_row_norm_max<DT, L>), dim3(grid_blocks(n, 256 / L, GRID_CAP)), dim3(256), 0, st, x, n, d, out));
        } else {
            hipLaunchKernelGGL((k_row_norm_max<DT, 64>), dim3(grid_blocks(n, 256 / 64, GRID_CAP)), dim3(256), 0, st, x, n, d, out);
        }
    });
    return check_launch("k_row_norm_max");
}

extern "C" int sss_f32_to_bf16(const float* x, int64_t count, uint16_t* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count < 0 || count % 8) { set_error("f32_to_bf16: element count must be a multiple of 8"); return SSS_EINVAL; }
    if (count == 0) return SSS_OK;
    hipLaunchKernelGGL(k_f32_to_bf16, dim3(grid_blocks(count / 8, 256, 4096)), dim3(256), 0, st, x, count / 8, y);
    return check_launch("k_f32_to_bf16");
}

extern "C" int sss_split_bf16(const float* x, int64_t n, int d, uint16_t* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d <= 0 || d % 8) { set_error("split_bf16: need n >= 0, d %% 8 == 0"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_split_bf16, dim3(grid_blocks(n * (d / 8), 256, 8192)), dim3(256), 0, st, x, n, d / 8, y);
    return check_launch("k_split_bf16");
}

extern "C" int sss_abs_max(const float* x, int64_t count, float* out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count < 0 || count % 4) { set_error("abs_max: element count must be a multiple of 4"); return SSS_EINVAL; }
    if (count == 0) return SSS_OK;
    hipLaunchKernelGGL(k_abs_max, dim3(grid_blocks(count / 4, 256, 4096)), dim3(256), 0, st, x, count / 4, out);
    return check_launch("k_abs_max");
}

extern "C" int sss_scale_f16(const float* x, int64_t count, int shift, uint16_t* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (count < 0 || count % 8) { set_error("scale_f16: element count must be a multiple of 8"); return SSS_EINVAL; }
    if (shift < -160 || shift > 160) { set_error("scale_f16: shift out of range"); return SSS_EINVAL; }
    if (count == 0) return SSS_OK;
    hipLaunchKernelGGL(k_scale_f16, dim3(grid_blocks(count / 8, 256, 8192)), dim3(256), 0, st, x, count / 8, shift, y);
    return check_launch("k_scale_f16");
}

extern "C" int sss_f16_resid_max(const float* x, const uint16_t* y, int64_t n, int d, int shift, float* out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d <= 0 || shift < -160 || shift > 160) { set_error("f16_resid_max: bad arguments"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_f16_resid_max, dim3(grid_blocks(n, 4, 16384)), dim3(256), 0, st, x, reinterpret_cast<const _Float16*>(y), n,
                       d, shift, out);
    return check_launch("k_f16_resid_max");
}

// the row-widening builders: d % 4 == 0, ds % 8 == 0, 0 < d <= ds <= 2^16; n == 0 is a no-op
static int check_pad_rows(const char* what, const void* x, const void* y, long n, int d, int ds) {
    if (n < 0 || d <= 0 || d % 4 || ds % 8 || d > ds || ds > 65536) {
        set_error("%s: need n >= 0, 0 < d <= ds, d %% 4 == 0, ds %% 8 == 0 (d %d, ds %d)", what, d, ds);
        return SSS_EINVAL;
    }
    if (n > 0 && (!aligned16(x) || !aligned16(y))) {
        set_error("%s: rows and output are required, 16-byte aligned", what);
        return SSS_EINVAL;
    }
    return SSS_OK;
}
static unsigned pad_grid(long chunks) { return grid_blocks(chunks, 256, 8192); }

extern "C" int sss_pad_rows_f32(const float* x, int64_t n, int d, int ds, float* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = check_pad_rows("pad_rows_f32", x, y, n, d, ds);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(k_pad_rows_f32, dim3(pad_grid(n * (ds / 4))), dim3(256), 0, st, x, n, d / 4, ds / 4, y);
    return check_launch("k_pad_rows_f32");
}

extern "C" int sss_pad_scale_f16(const float* x, int64_t n, int d, int ds, int shift, uint16_t* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = check_pad_rows("pad_scale_f16", x, y, n, d, ds);
    if (rc) return rc;
    if (shift < -160 || shift > 160) { set_error("pad_scale_f16: shift out of range"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_pad_scale_f16, dim3(pad_grid(n * (ds / 8))), dim3(256), 0, st, x, n, d / 4, ds / 8, shift, y);
    return check_launch("k_pad_scale_f16");
}

extern "C" int sss_pad_split_bf16(const float* x, int64_t n, int d, int ds, uint16_t* y, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = check_pad_rows("pad_split_bf16", x, y, n, d, ds);
    if (rc || n == 0) return rc;
    hipLaunchKernelGGL(k_pad_split_bf16, dim3(pad_grid(n * (ds / 8))), dim3(256), 0, st, x, n, d / 4, ds / 8, y);
    return check_launch("k_pad_split_bf16");
}

extern "C" int sss_pad_f16_resid_max(const float* x, const uint16_t* y, int64_t n, int d, int ds, int shift, float* out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rc = check_pad_rows("pad_f16_resid_max", x, y, n, d, ds);
    if (rc) return rc;
    if (shift < -160 || shift > 160 || (n > 0 && !out)) { set_error("pad_f16_resid_max: shift out of range or no output"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_pad_f16_resid_max, dim3(grid_blocks(n, 16, 16384)), dim3(256), 0, st, x, reinterpret_cast<const _Float16*>(y), n, d / 4,
                       ds / 8, shift, out);
    return check_launch("k_pad_f16_resid_max");
}

extern "C" int sss_l2_row_bias(const float* corpus, int64_t n, int d, float* bias, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d <= 0 || d % 4 || (n > 0 && (!corpus || !bias))) { set_error("l2_row_bias: need n >= 0, d %% 4 == 0, rows and bias"); return SSS_EINVAL; }
    if (n == 0) return SSS_OK;
    hipLaunchKernelGGL(k_row_bias, dim3(grid_blocks(n, 256 / 4, GRID_CAP)), dim3(256), 0, st, corpus, n, d, bias);
    return check_launch("k_row_bias");
}

extern "C" int sss_gather_rows(const float* table, const int64_t* ids, int64_t n, int d, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d <= 0 || d % 4 || ld_out < d || ld_out % 4) {
        set_error("gather_rows: need n >= 0, d %% 4 == 0, ld_out >= d, ld_out %% 4 == 0");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    const int lpr = lanes_for(d);
    SSS_LPR_SWITCH(lpr, hipLaunchKernelGGL(k_gather_rows<L>, dim3(grid_blocks(n, 256 / L, GRID_CAP)), dim3(256), 0, st, table, ids, n, d, out, ld_out));
    return check_launch("k_gather_rows");
}

extern "C" int sss_gather_concat_rows(const float* table, const int64_t* ids, int d_id, const float* feat, int64_t ld_feat, int d_feat,
                                      int d_pad, int64_t n, float* out, int64_t ld_out, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || d_id < 0 || d_feat < 0 || d_pad < 0 || d_id % 4 || d_feat % 4 || d_pad % 4 || d_id + d_feat + d_pad <= 0 ||
        ld_out % 4 || ld_out < d_id + d_feat + d_pad || (feat && (ld_feat % 4 || ld_feat < d_feat)) || (d_id > 0 && (!table || !ids))) {
        set_error("gather_concat_rows: need widths %% 4 == 0, ld_out >= d_id + d_f + d_pad, 16-byte aligned row strides");
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    const int lpr = lanes_for(d_id + d_feat + d_pad);
    SSS_LPR_SWITCH(lpr, hipLaunchKernelGGL(k_gather_concat_rows<L>, dim3(grid_blocks(n, 256 / L, GRID_CAP)), dim3(256), 0, st, table, ids, d_id, feat,
                                             ld_feat, d_feat, d_pad, n, out, ld_out));
    return check_launch("k_gather_concat_rows");
}

}  // namespace sss
