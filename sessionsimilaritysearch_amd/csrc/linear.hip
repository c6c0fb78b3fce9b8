// The grouped f32 GEMM every model runs its dense layers on (gfx950):
//   k_linear_grouped    Y[N, M] = act(X[N, K] W[M, K]^T + bias) (+ a per-column scale / shift / relu stage) for up to four
//                       problems in one launch: the node transforms inside PyG GATConv (lin_src), GatedGraphConv
//                       (x @ weight), torch GRUCell (W_ih, W_hh) and the nn.Linear layers of PositionalAttentionPooling
//                       (reference model/gnn.py:54,58,186-190), the conv / pool / head
//                       variants (variants.py) and the four GEMMs of a transformer layer (text.py)
//   sss_linear          one problem of it;  sss_linear_grouped  the launch as the callers see it (include/sss.h)
// Dense contractions run on v_mfma_f32_32x32x2_f32 (bit-exact f32 fma chains, the same rate as the f32 VALU peak).
#include "linear_dev.h"

namespace sss {

constexpr int LT = 64;      // GEMM tile rows (X) and columns (W rows): see k_linear_grouped below

template <int KC>
__global__ __launch_bounds__(256, 2) void k_linear_grouped(const LinBatch B) {
    constexpr int CPR = KC / 4;
    constexpr int NLD = LT * CPR / 256;
    constexpr int RS = CPR;                     // LDS row stride in 16-byte chunks
    constexpr int SW = RS < 16 ? RS - 1 : 15;   // XOR swizzle mask (stays inside the row)
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    float* lx = lds_raw;
    float* lw = lds_raw + LT * RS * 4;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i < B.nprob && (int)blockIdx.x >= B.s[i].tile_begin) pi = i;
    // copy the chosen problem's fields through scalar selects (no runtime-indexed struct access)
    const float* X = B.s[0].p.x; long ldx = B.s[0].p.ldx; const long* ids = B.s[0].p.ids; const float* table = B.s[0].p.table;
    float* xcopy = B.s[0].p.xcopy; long ldc = B.s[0].p.ld_xcopy; const float* W = B.s[0].p.w; long ldw = B.s[0].p.ldw;
    const float* bias = B.s[0].p.bias; float* Y = B.s[0].p.y; long ldy = B.s[0].p.ldy; long N = B.s[0].p.n; int M = B.s[0].p.m;
    int tiles_m = B.s[0].tiles_m, tile_begin = B.s[0].tile_begin, act = B.s[0].p.act;
    const float* post_s = B.s[0].p.post_scale; const float* post_t = B.s[0].p.post_shift;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (pi == i) {
            act = B.s[i].p.act; post_s = B.s[i].p.post_scale; post_t = B.s[i].p.post_shift;
            X = B.s[i].p.x; ldx = B.s[i].p.ldx; ids = B.s[i].p.ids; table = B.s[i].p.table; xcopy = B.s[i].p.xcopy; ldc = B.s[i].p.ld_xcopy;
            W = B.s[i].p.w; ldw = B.s[i].p.ldw; bias = B.s[i].p.bias; Y = B.s[i].p.y; ldy = B.s[i].p.ldy; N = B.s[i].p.n; M = B.s[i].p.m;
            tiles_m = B.s[i].tiles_m; tile_begin = B.s[i].tile_begin;
        }
    const int K = B.K;
    const int t = (int)blockIdx.x - tile_begin;
    const long row0 = (long)(t / tiles_m) * LT;
    const int col0 = (t % tiles_m) * LT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int xr = wr * 32 + r, wrow = wc * 32 + r;

    f32x16 acc = {0};
    f32x4 sx[NLD], sw[NLD];          // register staging of one K chunk (ext-vector type: stays in VGPRs)
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int p = tid + 256 * i;
            const int tr = p / CPR, c = p % CPR;
            long gr = row0 + tr; if (gr > N - 1) gr = N - 1;
            int gw = col0 + tr; if (gw > M - 1) gw = M - 1;
            const float* xrow = ids ? table + ids[gr] * (long)K : X + gr * ldx;
            sx[i] = *reinterpret_cast<const f32x4*>(xrow + k0 + c * 4);
            sw[i] = *reinterpret_cast<const f32x4*>(W + (long)gw * ldw + k0 + c * 4);
            if (ids && xcopy && col0 == 0 && row0 + tr < N)          // the gathered rows = slice 0 of the node buffer
                *reinterpret_cast<f32x4*>(xcopy + gr * ldc + k0 + c * 4) = sx[i];
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += KC) {
        if (k0 > 0) __syncthreads();                         // previous chunk fully consumed
#pragma unroll
        for (int i = 0; i < NLD; ++i) {
            const int p = tid + 256 * i;
            const int tr = p / CPR, c = p % CPR;
            const int cs = c ^ (tr & SW);
            *reinterpret_cast<f32x4*>(lx + (tr * RS + cs) * 4) = sx[i];
            *reinterpret_cast<f32x4*>(lw + (tr * RS + cs) * 4) = sw[i];
        }
        __syncthreads();
        if (k0 + KC < K) fetch(k0 + KC);                     // next chunk's loads fly under this chunk's MFMAs
        float4 a = *reinterpret_cast<const float4*>(lx + (xr * RS + (h ^ (xr & SW))) * 4);
        float4 b = *reinterpret_cast<const float4*>(lw + (wrow * RS + (h ^ (wrow & SW))) * 4);
#pragma unroll
        for (int u = 0; u < KC / 8; ++u) {
            float4 na = a, nb = b;
            if (u + 1 < KC / 8) {
                na = *reinterpret_cast<const float4*>(lx + (xr * RS + ((2 * u + 2 + h) ^ (xr & SW))) * 4);
                nb = *reinterpret_cast<const float4*>(lw + (wrow * RS + ((2 * u + 2 + h) ^ (wrow & SW))) * 4);
            }
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
            a = na; b = nb;
        }
    }
    const int col = col0 + wc * 32 + r;
    if (col < M) {
        const float bv = bias ? bias[col] : 0.f;
        const float ps = post_s ? post_s[col] : 1.f, pt = post_s ? post_t[col] : 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const long row = row0 + wr * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
            linear_epilogue(acc[j], bv, act, post_s, ps, pt, row, N, Y, ldy, col);
        }
    }
}

// ------------------------------------------------------------------------------ host launchers
static int linear_grouped(LinBatch& b, hipStream_t st) {
    if (b.nprob < 1 || b.nprob > 4 || b.K <= 0 || b.K % 32) { set_error("linear_grouped: 1..4 problems, K %% 32 == 0"); return SSS_EINVAL; }
    int total = 0;
    for (int i = 0; i < b.nprob; ++i) {
        const sss_linear_problem& p = b.s[i].p;
        if (p.n < 0 || p.m <= 0 || p.ldw % 4 || p.ldw < b.K || p.ldy < p.m || (!p.ids && (p.ldx % 4 || p.ldx < b.K)) ||
            (p.ids && (!p.table || (p.xcopy && (p.ld_xcopy % 4 || p.ld_xcopy < b.K))))) {
            set_error("linear_grouped: problem %d has bad strides / shapes", i);
            return SSS_EINVAL;
        }
        b.s[i].tiles_m = (p.m + LT - 1) / LT;
        b.s[i].tile_begin = total;
        total += (int)((p.n + LT - 1) / LT) * b.s[i].tiles_m;
    }
    for (int i = b.nprob; i < 4; ++i) { b.s[i] = b.s[0]; b.s[i].tile_begin = 0x7fffffff; }
    if (total == 0) return SSS_OK;
    // K chunks of 32: 16 KiB of LDS per workgroup, so eight workgroups share a CU, the whole grid of a
    // query-batch launch is resident at once and the load / MFMA / store phases of different workgroups
    // overlap (these launches are latency-bound, not FLOP-bound; measured against 64- and 128-chunks)
    const int lds32 = 2 * LT * 8 * 16;
    // (chunks of 64 on deep, chip-filling problems -- corpus build, the reference's 768 / 800-wide layers -- measured the same)
    hipLaunchKernelGGL(k_linear_grouped<32>, dim3((unsigned)total), dim3(256), lds32, st, b);
    return check_launch("k_linear_grouped");
}

// Y[N, M] = X[N, K] * W[M, K]^T (+ bias[M]): one problem of the grouped kernel (round 3: the separate 64 x 64
// kernel this entry point used to launch computed the identical fma chains 8-20 % slower on every shape).
extern "C" int sss_linear(const float* x, int64_t ldx, const float* w, int64_t ldw, const float* bias, float* y, int64_t ldy, int64_t n,
                          int m, int k, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (n < 0 || m <= 0 || k <= 0 || k % 32 || ldx % 4 || ldw % 4 || ldx < k || ldw < k || ldy < m) {
        set_error("linear: need K %% 32 == 0, ldx/ldw %% 4 == 0 and >= K, ldy >= M (N=%ld M=%d K=%d)", n, m, k);
        return SSS_EINVAL;
    }
    if (n == 0) return SSS_OK;
    LinBatch b = {};
    b.nprob = 1; b.K = k;
    sss_linear_problem& p = b.s[0].p;                          // every other field stays null / 0
    p.x = x; p.ldx = ldx; p.w = w; p.ldw = ldw; p.bias = bias; p.y = y; p.ldy = ldy; p.n = n; p.m = m;
    return linear_grouped(b, st);
}

extern "C" int sss_linear_grouped(const sss_linear_problem* problems, int n_problems, int k, void* stream) {
    if (!problems || n_problems < 1 || n_problems > 4) { set_error("linear_grouped: 1..4 problems"); return SSS_EINVAL; }
    LinBatch b;
    b.nprob = n_problems; b.K = k;
    for (int i = 0; i < n_problems; ++i) {
        b.s[i].p = problems[i];
        const sss_linear_problem& p = b.s[i].p;
        if (p.act < 0 || p.act > 5 || (p.post_scale == nullptr) != (p.post_shift == nullptr)) {
            set_error("linear_grouped: problem %d: act must be 0..5, post_scale / post_shift come together", i);
            return SSS_EINVAL;
        }
    }
    return linear_grouped(b, static_cast<hipStream_t>(stream));
}

}  // namespace sss
