// The catalogue heads (gfx950): the model's own item prediction over the whole catalogue, include/heads/sss_catalogue.h.
//   k_catalogue_bce        rep[B, Kp] . table[V, Kp]^T on v_mfma_f32_32x32x2_f32 in k_linear_grouped's tile and k order (the
//                          logit is the same bits as sss_linear's output), with the loss terms taken from the accumulators
//                          on the vector pipe: the [B, V] matrix of the reference's get_next / get_all_product_asin_loss
//                          (train_subsession_embedding.py:271-302, train_session_embedding.py:122-) never exists.  One
//                          workgroup owns 64 rows and a span of SSS_CATALOGUE_SPAN items and writes one partial per row
//   k_catalogue_finish     adds a row's partials in ascending span order
//   k_catalogue_hits       distinct entries of a top-K row that lie in the row's target set
#include "sss_common.h"
#include "../../include/heads/sss_catalogue.h"

namespace sss {

constexpr int CT = 64;                              // tile rows (sessions) and tile columns (items), as k_linear_grouped
static_assert(SSS_CATALOGUE_SPAN % CT == 0, "a span is whole tiles");

// first index in [lo, hi) whose item is >= key (items ascending there)
__device__ __forceinline__ long lower_bound_items(const int* items, long lo, long hi, long key) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        if (items[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// H of the header from x = seed + (g * V + i) * 0x9E3779B97F4A7C15
__device__ __forceinline__ uint32_t splitmix_hi(uint64_t x) {
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    x = x ^ (x >> 31);
    return (uint32_t)(x >> 32);
}

// clamp(softplus(z), lo, hi); a NaN passes through both comparisons
__device__ __forceinline__ float bce_term(float z, float lo, float hi) {
    const float t = fmaxf(z, 0.f) + log1pf(expf(-fabsf(z)));
    return t < lo ? lo : (t > hi ? hi : t);
}

struct CatArgs {
    const float* rep; const float* table; long ldw; int Kp;
    const long* ptr; const int* items; long B; int V; int mode; uint32_t thr; uint64_t seed; long row_offset;
    double* psum; int* pcnt;           // [spans][B][2] partials
};

__global__ __launch_bounds__(256, 2) void k_catalogue_bce(const CatArgs A) {
    constexpr int KC = 32, CPR = KC / 4, NLD = CT * CPR / 256, RS = CPR, SW = RS - 1;
    __shared__ __attribute__((aligned(16))) float lx[CT * KC];
    __shared__ __attribute__((aligned(16))) float lw[CT * KC];
    __shared__ long t_beg[2][CT];      // per tile parity and row: where the row's targets inside the tile start ...
    __shared__ int t_cnt[2][CT];       // ... and how many there are
    __shared__ int t_any[2];           // whether any row has one (almost never)
    __shared__ double red_s[2][CT][2];
    __shared__ int red_c[2][CT][2];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    const int r = lane & 31, h = lane >> 5;
    const int xr = wr * 32 + r, wrow = wc * 32 + r;
    const long row0 = (long)blockIdx.y * CT;
    const int V = A.V, K = A.Kp;
    const long B = A.B;
    const long span0 = (long)blockIdx.x * SSS_CATALOGUE_SPAN;               // (long: v may end just below 2^31)
    const long span1 = min((long)V, span0 + SSS_CATALOGUE_SPAN);
    const int ntile = (int)((span1 - span0 + CT - 1) / CT);

    // wave 0, one lane per row: the row's targets inside this span (two binary searches, once per workgroup), walked
    // forward tile by tile below
    long cur = 0, end = 0;
    if (tid < CT && row0 + tid < B) {
        const long p0 = A.ptr[row0 + tid], p1 = A.ptr[row0 + tid + 1];
        cur = lower_bound_items(A.items, p0, p1, span0);
        end = lower_bound_items(A.items, cur, p1, span1);
    }

    // counter part of the hash that belongs to the row: seed + g * V * GOLDEN, per accumulator register
    const uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;
    const uint64_t VG = (uint64_t)V * GOLDEN;
    const uint64_t g0 = (uint64_t)(A.row_offset + row0 + wr * 32 + 4 * h);
    const uint64_t rb0 = A.seed + g0 * VG;

    double psum[16], nsum[16];
    int pcnt[16], ncnt[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) { psum[j] = 0.0; nsum[j] = 0.0; pcnt[j] = 0; ncnt[j] = 0; }

    for (int tt = 0; tt < ntile; ++tt) {
        const long col0 = span0 + tt * CT;
        const int par = tt & 1;
        if (tid < CT) {
            const long beg = cur;
            while (cur < end && A.items[cur] < col0 + CT) ++cur;
            t_beg[par][tid] = beg;
            t_cnt[par][tid] = (int)(cur - beg);
            const bool any = __ballot(cur > beg) != 0;
            if (tid == 0) t_any[par] = any;
        }
        f32x16 acc = {0};
        f32x4 sx[NLD], sw[NLD];
        auto fetch = [&](int k0) {
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int p = tid + 256 * i;
                const int tr = p / CPR, c = p % CPR;
                long gr = row0 + tr; if (gr > B - 1) gr = B - 1;
                long gw = col0 + tr; if (gw > V - 1) gw = V - 1;
                sx[i] = *reinterpret_cast<const f32x4*>(A.rep + gr * (long)K + k0 + c * 4);
                sw[i] = *reinterpret_cast<const f32x4*>(A.table + gw * A.ldw + k0 + c * 4);
            }
        };
        fetch(0);
        for (int k0 = 0; k0 < K; k0 += KC) {
            __syncthreads();                                     // previous chunk (or tile) fully consumed
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int p = tid + 256 * i;
                const int tr = p / CPR, c = p % CPR;
                const int cs = c ^ (tr & SW);
                *reinterpret_cast<f32x4*>(lx + (tr * RS + cs) * 4) = sx[i];
                *reinterpret_cast<f32x4*>(lw + (tr * RS + cs) * 4) = sw[i];
            }
            __syncthreads();
            if (k0 + KC < K) fetch(k0 + KC);
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
        // the loss terms of this lane's item against its 16 rows (the tile's target table was written before the K
        // loop's barriers; the next tile writes the other parity)
        const long item = col0 + wc * 32 + r;
        const bool item_ok = item < V;
        const uint64_t iG = (uint64_t)item * GOLDEN;
        const bool any_target = __builtin_amdgcn_readfirstlane(t_any[par]) != 0;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int dr = (j & 3) + 8 * (j >> 2);                       // row inside the wave's 32, beside 4 * h
            const int rl = wr * 32 + dr + 4 * h;
            bool pos = false;
            if (any_target) {
                const long beg = t_beg[par][rl];
                const int n = t_cnt[par][rl];
                for (int i = 0; i < n; ++i) pos |= A.items[beg + i] == item;
            }
            bool keep = pos || A.mode == 1;
            if (!keep) keep = splitmix_hi(rb0 + (uint64_t)dr * VG + iG) < A.thr;
            if (keep && item_ok && row0 + rl < B) {
                if (pos) { psum[j] += (double)bce_term(-acc[j], SSS_CATALOGUE_P_LO, SSS_CATALOGUE_P_HI); ++pcnt[j]; }
                else { nsum[j] += (double)bce_term(acc[j], SSS_CATALOGUE_N_LO, SSS_CATALOGUE_N_HI); ++ncnt[j]; }
            }
        }
    }

    // one partial per row: the 32 item lanes in a fixed butterfly, then the two column waves in order
#pragma unroll
    for (int j = 0; j < 16; ++j) {
#pragma unroll
        for (int m = 1; m < 32; m <<= 1) {
            psum[j] += __shfl_xor(psum[j], m);
            nsum[j] += __shfl_xor(nsum[j], m);
            pcnt[j] += __shfl_xor(pcnt[j], m);
            ncnt[j] += __shfl_xor(ncnt[j], m);
        }
        if (r == 0) {
            const int rl = wr * 32 + (j & 3) + 8 * (j >> 2) + 4 * h;
            red_s[wc][rl][0] = psum[j]; red_s[wc][rl][1] = nsum[j];
            red_c[wc][rl][0] = pcnt[j]; red_c[wc][rl][1] = ncnt[j];
        }
    }
    __syncthreads();
    if (tid < 2 * CT) {
        const int rl = tid >> 1, q = tid & 1;
        if (row0 + rl < B) {
            const long o = ((long)blockIdx.x * B + row0 + rl) * 2 + q;
            A.psum[o] = red_s[0][rl][q] + red_s[1][rl][q];
            A.pcnt[o] = red_c[0][rl][q] + red_c[1][rl][q];
        }
    }
}

// sums[r][q] / counts[r][q]: the row's partials in ascending span order
__global__ void k_catalogue_finish(const double* psum, const int* pcnt, long B, int spans, double* sums, long* counts) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;       // (row, q)
    if (i >= 2 * B) return;
    double s = 0.0;
    long c = 0;
    for (int sp = 0; sp < spans; ++sp) {
        s += psum[(long)sp * 2 * B + i];
        c += pcnt[(long)sp * 2 * B + i];
    }
    sums[i] = s;
    counts[i] = c;
}

__global__ __launch_bounds__(256) void k_catalogue_hits(const long* I, int K, const long* ptr, const int* items, int* hits) {
    __shared__ int total;
    const long b = blockIdx.x;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long p0 = ptr[b], p1 = ptr[b + 1];
    const long* row = I + b * K;
    int mine = 0;
    for (int j = threadIdx.x; j < K; j += 256) {
        const long id = row[j];
        if (id < 0 || id > 0x7fffffffL) continue;
        const long p = lower_bound_items(items, p0, p1, id);
        if (p < p1 && items[p] == id) {
            bool first = true;
            for (int e = 0; e < j && first; ++e) first = row[e] != id;
            mine += first;
        }
    }
    if (mine) atomicAdd(&total, mine);
    __syncthreads();
    if (threadIdx.x == 0) hits[b] = total;
}

static long spans_of(long v) { return (v + SSS_CATALOGUE_SPAN - 1) / SSS_CATALOGUE_SPAN; }
constexpr long CAT_MAX_B = 65535L * CT;

extern "C" size_t sss_catalogue_bce_workspace_bytes(int64_t b, int64_t v) {
    if (b <= 0 || v <= 0) return 256;
    const size_t cells = (size_t)spans_of(v) * (size_t)b * 2;
    return al256(cells * sizeof(double)) + al256(cells * sizeof(int));
}

extern "C" int sss_catalogue_bce(const float* rep, const float* table, int64_t ldw, int kp, const int64_t* ptr, const int32_t* items,
                                 int64_t b, int64_t v, int mode, uint32_t keep_thr, uint64_t seed, int64_t row_offset, double* sums,
                                 int64_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
    if (kp <= 0 || kp % 32 || ldw % 4 || ldw < kp) { set_error("catalogue_bce: need kp %% 32 == 0, ldw %% 4 == 0 and ldw >= kp (kp=%d ldw=%ld)", kp, ldw); return SSS_EINVAL; }
    if (v <= 0 || v > 0x7fffffffL) { set_error("catalogue_bce: need 0 < v < 2^31 (v=%ld)", v); return SSS_EINVAL; }
    if (b < 0 || b > CAT_MAX_B) { set_error("catalogue_bce: need 0 <= b <= %ld (b=%ld)", CAT_MAX_B, b); return SSS_EINVAL; }
    if (mode != 0 && mode != 1) { set_error("catalogue_bce: mode must be 0 (hashed negatives) or 1 (all negatives), got %d", mode); return SSS_EINVAL; }
    if (row_offset < 0) { set_error("catalogue_bce: row_offset must be >= 0 (got %ld)", row_offset); return SSS_EINVAL; }
    if (b == 0) return SSS_OK;
    if (!rep || !table || !ptr || !items || !sums || !counts) { set_error("catalogue_bce: rep, table, ptr, items, sums and counts must not be null"); return SSS_EINVAL; }
    const size_t need = sss_catalogue_bce_workspace_bytes(b, v);
    if (!workspace || workspace_bytes < need) { set_error("catalogue_bce: workspace of %zu bytes, %zu needed", workspace ? workspace_bytes : (size_t)0, need); return SSS_EWORKSPACE; }
    if (reinterpret_cast<uintptr_t>(workspace) % 8) { set_error("catalogue_bce: workspace must be 8-byte aligned"); return SSS_EINVAL; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long spans = spans_of(v);
    CatArgs a;
    a.rep = rep; a.table = table; a.ldw = ldw; a.Kp = kp; a.ptr = ptr; a.items = items; a.B = b; a.V = (int)v; a.mode = mode;
    a.thr = keep_thr; a.seed = seed; a.row_offset = row_offset;
    a.psum = static_cast<double*>(workspace);
    a.pcnt = reinterpret_cast<int*>(static_cast<char*>(workspace) + al256((size_t)spans * (size_t)b * 2 * sizeof(double)));
    hipLaunchKernelGGL(k_catalogue_bce, dim3((unsigned)spans, (unsigned)((b + CT - 1) / CT)), dim3(256), 0, st, a);
    int rc = check_launch("k_catalogue_bce");
    if (rc) return rc;
    hipLaunchKernelGGL(k_catalogue_finish, dim3((unsigned)((2 * b + 255) / 256)), dim3(256), 0, st, a.psum, a.pcnt, (long)b, (int)spans, sums, counts);
    return check_launch("k_catalogue_finish");
}

extern "C" int sss_catalogue_hits(const int64_t* I, int64_t b, int k, const int64_t* ptr, const int32_t* items, int32_t* hits, void* stream) {
    if (k <= 0 || k > 1024) { set_error("catalogue_hits: need 0 < k <= 1024 (k=%d)", k); return SSS_EINVAL; }
    if (b < 0 || b > 0x7fffffffL) { set_error("catalogue_hits: need 0 <= b < 2^31 (b=%ld)", b); return SSS_EINVAL; }
    if (b == 0) return SSS_OK;
    if (!I || !ptr || !items || !hits) { set_error("catalogue_hits: I, ptr, items and hits must not be null"); return SSS_EINVAL; }
    hipLaunchKernelGGL(k_catalogue_hits, dim3((unsigned)b), dim3(256), 0, static_cast<hipStream_t>(stream), I, k, ptr, items, hits);
    return check_launch("k_catalogue_hits");
}

}  // namespace sss
