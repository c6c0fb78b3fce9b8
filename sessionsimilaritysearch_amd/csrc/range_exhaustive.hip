// RANGE SEARCH, exhaustive route: the canonical scores of the selected queries against every row (exhaustive.hip:
// launch_exact_scores), then, per query, the rows that pass -- score > radius (metric 0) or distance < radius (metric 1),
// strict -- counted per slab and compacted in id order (slab_compact.h under KeepRange).  The count and the fill are two
// calls (the caller sizes the output in between); the scores stay in the workspace from one to the other.
// Workspace: scores f32 [nsel][n] | (256-byte aligned) slab offsets u32 [nsel][nslabs].
#include "scan.h"
#include "slab_compact.h"

namespace sss {

constexpr int RG_SLAB = 16384;        // rows per counting / compaction workgroup
constexpr int RG_THREADS = 256;

static long rg_slabs(long n) { return (n + RG_SLAB - 1) / RG_SLAB; }

// THE RANGE KEEP: one flag, the rows that pass the query's radius.  A passing row
// goes to D / I at lims[f] + (passing rows before it).  Every write stays inside [lims[f], lims[f + 1]) and below
// lims[nsel] (the size of D / I) whatever lims holds.
struct KeepRange {
    static constexpr int F = 1, SLAB = RG_SLAB, COUNT_THREADS = RG_THREADS, COMPACT_THREADS = RG_THREADS;
    const float* scores;
    long n;
    int metric;
    const float* radius;
    const int* qsel;
    int nsel;
    const long* lims;
    long id_offset;
    float* D;
    long* I;
    float r;
    long q_lo, q_hi;
    __device__ void load(int f) { r = radius[qsel[f]]; }
    __device__ bool open(int f) {
        const long total = lims[nsel];
        q_lo = lims[f];
        q_hi = lims[f + 1];
        if (q_hi > total) q_hi = total;
        return !(q_lo < 0 || q_lo >= q_hi);
    }
    __device__ void classify(float s, bool (&flag)[1]) const { flag[0] = metric == 0 ? s > r : s < r; }
    __device__ void emit(const bool (&flag)[1], const unsigned (&before)[1], float v, long row) const {
        const long pos = q_lo + (long)before[0];
        if (flag[0] && pos < q_hi) { D[pos] = v; I[pos] = row + id_offset; }
    }
};

__global__ __launch_bounds__(RG_THREADS) void k_range_count(const float* __restrict__ scores, long n, int metric,
                                                            const float* __restrict__ radius, const int* __restrict__ qsel, int nslabs,
                                                            unsigned* __restrict__ cnt) {
    slab_count(KeepRange{scores, n, metric, radius, qsel}, nslabs, {cnt});
}

// one thread per query: exclusive scan of its slab counts (in place) and its total
__global__ __launch_bounds__(64) void k_range_scan(unsigned* __restrict__ cnt, int nslabs, int nsel, long* __restrict__ counts) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= nsel) return;
    unsigned run = 0;
    for (int j = 0; j < nslabs; ++j) {
        const unsigned c = cnt[(size_t)f * nslabs + j];
        cnt[(size_t)f * nslabs + j] = run;
        run += c;
    }
    counts[f] = (long)run;
}

__global__ __launch_bounds__(RG_THREADS) void k_range_compact(const float* __restrict__ scores, long n, int metric,
                                                              const float* __restrict__ radius, const int* __restrict__ qsel, int nslabs,
                                                              const unsigned* __restrict__ off, int nsel, const long* __restrict__ lims,
                                                              long id_offset, float* __restrict__ D, long* __restrict__ I) {
    slab_compact(KeepRange{scores, n, metric, radius, qsel, nsel, lims, id_offset, D, I}, nslabs, {off});
}

extern "C" size_t sss_range_search_exhaustive_workspace_bytes(int64_t nsel, int64_t n) {
    if (nsel <= 0 || n <= 0) return 0;
    return score_matrix_bytes(nsel, n) + al256((size_t)nsel * rg_slabs(n) * 4);
}

static int range_exhaustive_check(const char* what, const int* qsel, long nsel, long n, int metric, const float* radius, const void* ws,
                                  size_t ws_bytes) {
    if (nsel <= 0 || n <= 0 || (metric != 0 && metric != 1) || !qsel || !radius) {
        set_error("%s: need nsel, n > 0, metric in {0,1}, qsel and radius", what);
        return SSS_EINVAL;
    }
    if (n >= (1L << 31) || nsel > 65535) { set_error("%s: n < 2^31, nsel <= 65535", what); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(ws) & 255) { set_error("%s: workspace must be 256-byte aligned", what); return SSS_EINVAL; }
    if (!ws || ws_bytes < sss_range_search_exhaustive_workspace_bytes(nsel, n)) {
        set_error("%s: workspace %zu < %zu", what, ws_bytes, sss_range_search_exhaustive_workspace_bytes(nsel, n));
        return SSS_EWORKSPACE;
    }
    return SSS_OK;
}

extern "C" int sss_range_search_exhaustive_count(const void* q, const int32_t* qsel, int64_t nsel, const void* corpus, int64_t n, int d,
                                                 int dtype, int metric, const float* radius, int64_t* counts, void* workspace,
                                                 size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d <= 0 || !corpus_dtype_ok(dtype) || d % elems_per_chunk(dtype) || !q || !corpus || !counts) {
        set_error("range_exhaustive_count: need %s, q, corpus and counts", row_align_text());
        return SSS_EINVAL;
    }
    int rc = range_exhaustive_check("range_exhaustive_count", qsel, nsel, n, metric, radius, workspace, workspace_bytes);
    if (rc) return rc;
    float* scores = reinterpret_cast<float*>(workspace);
    unsigned* cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(workspace) + score_matrix_bytes(nsel, n));
    const int nslabs = (int)rg_slabs(n);
    // inner product: the radius is a valid pre-test bound -- a row k_exact_scores_rows skips (score -FLT_MAX) provably
    // rounds to at most the radius, so it fails "> radius" either way
    rc = launch_exact_scores(q, qsel, nsel, corpus, n, d, dtype, metric, scores, metric == 0 ? radius : nullptr, 1, st);
    if (rc) return rc;
    hipLaunchKernelGGL(k_range_count, dim3((unsigned)nslabs, (unsigned)nsel), dim3(RG_THREADS), 0, st, scores, n, metric, radius, qsel,
                       nslabs, cnt);
    rc = check_launch("k_range_count");
    if (rc) return rc;
    hipLaunchKernelGGL(k_range_scan, dim3((unsigned)((nsel + 63) / 64)), dim3(64), 0, st, cnt, nslabs, (int)nsel, counts);
    return check_launch("k_range_scan");
}

extern "C" int sss_range_search_exhaustive_fill(const int32_t* qsel, int64_t nsel, int64_t n, int metric, const float* radius,
                                                const int64_t* lims, int64_t id_offset, float* D_out, int64_t* I_out,
                                                const void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    int rc = range_exhaustive_check("range_exhaustive_fill", qsel, nsel, n, metric, radius, workspace, workspace_bytes);
    if (rc) return rc;
    if (!lims) { set_error("range_exhaustive_fill: lims is required"); return SSS_EINVAL; }
    const float* scores = reinterpret_cast<const float*>(workspace);
    const unsigned* off = reinterpret_cast<const unsigned*>(reinterpret_cast<const char*>(workspace) + score_matrix_bytes(nsel, n));
    const int nslabs = (int)rg_slabs(n);
    hipLaunchKernelGGL(k_range_compact, dim3((unsigned)nslabs, (unsigned)nsel), dim3(RG_THREADS), 0, st, scores, n, metric, radius, qsel,
                       nslabs, off, (int)nsel, lims, id_offset, D_out, I_out);
    return check_launch("k_range_compact");
}

}  // namespace sss
