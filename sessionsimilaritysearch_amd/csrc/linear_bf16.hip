// The reduced-precision grouped GEMM (gfx950), opt-in beside k_linear_grouped (linear.hip):
//   k_linear_grouped_bf16    Y[N, M] = act(bf16(X)[N, K] Wb[M, K]^T + bias) (+ the per-column scale / shift / relu stage) for up
//                            to four problems in one launch.  X is float32 in memory and is rounded to bfloat16 (round to
//                            nearest even: the plain cast, as k_f32_to_bf16 of rowops.hip) on its way into LDS; Wb is bf16
//                            in memory; the sum is float32 on v_mfma_f32_32x32x16_bf16; bias, activation, post stage and
//                            the store are linear_epilogue (linear_dev.h), the float32 arithmetic of k_linear_grouped.
//   sss_linear_grouped_bf16  the launch as the callers see it (include/lowp/sss_linear_bf16.h: limits, error contract)
// text.py runs the dense layers of BertNodeEncoder / NodeTextTransformer on it under gemm="bf16" (DESIGN.md section 5.10).
//
// Geometry.  256 threads, a 128 x 128 output tile, four waves of 64 x 64 each: 2 x 2 accumulators of 32 x 32 (64 VGPRs).
// K is walked in chunks of 64: the X tile and the W tile are [128][64] bf16 images in LDS (16 KiB each, 128-byte rows),
// double-buffered through registers as k_linear_grouped does -- the next chunk's global loads fly under this chunk's MFMAs
// and are converted and written after the barrier that retires this chunk's reads.  Per chunk a wave issues 16 MFMAs and
// 16 ds_read_b128 (two X and two W fragments per 16-deep k step): one read per MFMA.
// LDS layout.  The 16-byte chunk c (0..7) of row r is stored at chunk c ^ ((r >> 1) & 7).  A ds_read_b128 is served in four
// groups of 16 lanes over a 256-byte bank row, i.e. two image rows: a group's lanes read one chunk c of 16 rows r that
// are (in the hardware's grouping) two aligned runs of 4 and one of 8, so their (r & 1, (r >> 1) & 7) pairs are all
// different and the 16 reads land on 16 different 16-byte slots: conflict-free.  The staging stores use the same formula.
// The order of the sum is fixed by K alone: k ascending in steps of 16, each step one MFMA (zero-padded to a whole chunk
// when K % 64 == 32, which adds exact zeros), the same for every row, column, tile and problem.
#include "linear_bf16_plan.h"
#include "linear_dev.h"
#include "../../include/lowp/sss_linear_bf16.h"

namespace sss {

constexpr int BF_K = 64;     // K chunk in bf16 elements
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256, 2) void k_linear_grouped_bf16(const LinBatch B) {
    __shared__ __attribute__((aligned(16))) unsigned short lds[2 * BF_T * BF_K];
    unsigned short* lx = lds;
    unsigned short* lw = lds + BF_T * BF_K;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i < B.nprob && (int)blockIdx.x >= B.s[i].tile_begin) pi = i;
    // copy the chosen problem's fields through scalar selects (no runtime-indexed struct access)
    const float* X = B.s[0].p.x; long ldx = B.s[0].p.ldx; const float* Wf = B.s[0].p.w; long ldw = B.s[0].p.ldw;
    const float* bias = B.s[0].p.bias; float* Y = B.s[0].p.y; long ldy = B.s[0].p.ldy; long N = B.s[0].p.n; int M = B.s[0].p.m;
    int tiles_m = B.s[0].tiles_m, tile_begin = B.s[0].tile_begin, act = B.s[0].p.act;
    const float* post_s = B.s[0].p.post_scale; const float* post_t = B.s[0].p.post_shift;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (pi == i) {
            act = B.s[i].p.act; post_s = B.s[i].p.post_scale; post_t = B.s[i].p.post_shift;
            X = B.s[i].p.x; ldx = B.s[i].p.ldx; Wf = B.s[i].p.w; ldw = B.s[i].p.ldw;
            bias = B.s[i].p.bias; Y = B.s[i].p.y; ldy = B.s[i].p.ldy; N = B.s[i].p.n; M = B.s[i].p.m;
            tiles_m = B.s[i].tiles_m; tile_begin = B.s[i].tile_begin;
        }
    const unsigned short* W = reinterpret_cast<const unsigned short*>(Wf);       // bf16 bits, ldw in bf16 elements
    const int K = B.K;
    const int t = (int)blockIdx.x - tile_begin;
    const long row0 = (long)(t / tiles_m) * BF_T;
    const int col0 = (t % tiles_m) * BF_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 31, h = lane >> 5;

    // staging: thread (tr0, c8) moves the 8 elements [8 c8, 8 c8 + 8) of the chunk for rows tr0, tr0 + 32, tr0 + 64, tr0 + 96
    const int c8 = tid & 7, tr0 = tid >> 3;
    const float* xp[4];
    const unsigned short* wp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        long gr = row0 + tr0 + 32 * i; if (gr > N - 1) gr = N - 1;          // rows past the edge re-read the last one:
        int gw = col0 + tr0 + 32 * i; if (gw > M - 1) gw = M - 1;            // their results are never stored
        xp[i] = X + gr * ldx;
        wp[i] = W + (long)gw * ldw;
    }
    f32x4 sx[8];                     // register staging of one K chunk (ext-vector types: stay in VGPRs)
    u32x4 sw[4];
    auto fetch = [&](int k0) {
        int kk = k0 + c8 * 8; if (kk > K - 8) kk = K - 8;                   // K % 64 == 32: the last chunk's upper half is
#pragma unroll                                                               // loaded in bounds and zeroed below
        for (int i = 0; i < 4; ++i) {
            sx[2 * i] = *reinterpret_cast<const f32x4*>(xp[i] + kk);
            sx[2 * i + 1] = *reinterpret_cast<const f32x4*>(xp[i] + kk + 4);
            sw[i] = *reinterpret_cast<const u32x4*>(wp[i] + kk);
        }
    };
    const int st_off = (tr0 * 8 + (c8 ^ ((tr0 >> 1) & 7))) * 8;             // + 32 rows: the same swizzle (32 % 16 == 0)
    const int rd_sw = (r >> 1) & 7;                                         // every fragment row is r + a multiple of 32
    const int ax = ((wr * 64 + r) * 8) * 8, bx = ((wc * 64 + r) * 8) * 8;

    f32x16 acc[2][2] = {};
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += BF_K) {
        if (k0 > 0) __syncthreads();                         // previous chunk fully consumed
        const bool pad = k0 + BF_K > K && c8 >= 4;           // beyond K: exact zeros on both sides
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const f32x4 a = sx[2 * i], b = sx[2 * i + 1];
            bf16x8 o;
            o[0] = (__bf16)a.x; o[1] = (__bf16)a.y; o[2] = (__bf16)a.z; o[3] = (__bf16)a.w;
            o[4] = (__bf16)b.x; o[5] = (__bf16)b.y; o[6] = (__bf16)b.z; o[7] = (__bf16)b.w;
            u32x4 xo = __builtin_bit_cast(u32x4, o), wo = sw[i];
            if (pad) { xo = u32x4{0, 0, 0, 0}; wo = u32x4{0, 0, 0, 0}; }
            *reinterpret_cast<u32x4*>(lx + st_off + i * 32 * BF_K) = xo;
            *reinterpret_cast<u32x4*>(lw + st_off + i * 32 * BF_K) = wo;
        }
        __syncthreads();
        if (k0 + BF_K < K) fetch(k0 + BF_K);                 // next chunk's loads fly under this chunk's MFMAs
#pragma unroll
        for (int s = 0; s < BF_K / 16; ++s) {
            const int co = ((2 * s + h) ^ rd_sw) * 8;
            bf16x8 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = *reinterpret_cast<const bf16x8*>(lx + ax + i * 32 * BF_K + co);
                b[i] = *reinterpret_cast<const bf16x8*>(lw + bx + i * 32 * BF_K + co);
            }
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int ni = 0; ni < 2; ++ni)
                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[mi], b[ni], acc[mi][ni], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ni = 0; ni < 2; ++ni) {
        const int col = col0 + wc * 64 + ni * 32 + r;
        if (col < M) {
            const float bv = bias ? bias[col] : 0.f;
            const float ps = post_s ? post_s[col] : 1.f, pt = post_s ? post_t[col] : 0.f;
#pragma unroll
            for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const long row = row0 + wr * 64 + mi * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
                    linear_epilogue(acc[mi][ni][j], bv, act, post_s, ps, pt, row, N, Y, ldy, col);
                }
        }
    }
}

extern "C" int sss_linear_grouped_bf16(const sss_linear_problem* problems, int n_problems, int k, void* stream) {
    LinBatch b;
    int tiles_m[4], tile_begin[4], total = 0;
    char msg[160];
    if (!linear_bf16_plan(problems, n_problems, k, tiles_m, tile_begin, &total, msg, sizeof msg)) {
        set_error("%s", msg);
        return SSS_EINVAL;
    }
    b.nprob = n_problems; b.K = k;
    for (int i = 0; i < 4; ++i) {
        b.s[i].p = problems[i < n_problems ? i : 0];
        b.s[i].tiles_m = tiles_m[i < n_problems ? i : 0];
        b.s[i].tile_begin = i < n_problems ? tile_begin[i] : 0x7fffffff;
    }
    if (total == 0) return SSS_OK;
    hipLaunchKernelGGL(k_linear_grouped_bf16, dim3((unsigned)total), dim3(256), 0, static_cast<hipStream_t>(stream), b);
    return check_launch("k_linear_grouped_bf16");
}

}  // namespace sss
