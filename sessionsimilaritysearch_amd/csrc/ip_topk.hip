// Host orchestration of sss_ip_topk / sss_ip_topk_f16 / sss_ip_topk_split: plan -> k_scan (over the
// corpus or its f16 / split image) -> k_select_* (over the stored rows): two launches; the per-query
// state words are handed back zeroed by the select kernel, so there is no per-call memset.
// (reference call site: `D, I = index.search(normalize(emb), K)`, test_amazon_filterd.py:578.)
#include "scan.h"

namespace sss {

// Optional timing of the dominant kernel (bench.py roofline leg): when enabled, every k_scan
// launch is bracketed by a hipEvent pair on ITS stream; sss_profile_read() drains the ring of the
// calling thread's current device.
namespace {
constexpr int PROF_RING = 512;
struct Prof {
    bool on = false;
    int n = 0;
    hipEvent_t ev[2 * PROF_RING];
    bool made = false;
};
Prof g_prof[MAX_DEVICES];
}  // namespace

extern "C" int sss_profile_enable(int on) {
    Prof& p = g_prof[current_device()];
    if (on && !p.made) {
        for (int i = 0; i < 2 * PROF_RING; ++i)
            if (hipEventCreate(&p.ev[i]) != hipSuccess) { set_error("profile_enable: hipEventCreate failed"); return SSS_EHIP; }
        p.made = true;
    }
    p.on = on != 0;
    p.n = 0;
    return SSS_OK;
}

extern "C" int sss_profile_read(double* total_ms, int* launches) {
    Prof& p = g_prof[current_device()];
    double sum = 0.0;
    for (int i = 0; i < p.n; ++i) {
        if (hipEventSynchronize(p.ev[2 * i + 1]) != hipSuccess) { set_error("profile_read: sync failed"); return SSS_EHIP; }
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.ev[2 * i], p.ev[2 * i + 1]) != hipSuccess) { set_error("profile_read: elapsed failed"); return SSS_EHIP; }
        sum += ms;
    }
    *total_ms = sum;
    *launches = p.n;
    p.n = 0;
    return SSS_OK;
}

static bool fused_shape_ok(int d, int dtype) {
    const int rb = d * elem_bytes(dtype);
    // (DT_I8: d = 256 / 512 / 1024 -- the d <= 1024 that keeps an int8 score exact in float32, select_dev.h: err_bound)
    return format_of(dtype) && (rb == 256 || rb == 512 || rb == 1024);
}

// scan_dtype: what k_scan reads for rows of exact_dtype (elem.h: scan_pair_ok).
int check_scan_source(const char* what, int exact_dtype, int scan_dtype, int d, bool long_rows, const void* c_scan, int corpus_shift,
                      float corpus_resid, long n, long nq) {
    if (long_rows && exact_dtype == DT_I8) {
        set_error("%s: int8 rows (dtype %d) have no long-row scan: d in {256,512,1024} on the fused scan, else the exhaustive kernels", what, DT_I8);
        return SSS_EINVAL;
    }
    if (!(long_rows ? long_shape_ok(d, exact_dtype, scan_dtype) : scan_pair_ok(exact_dtype, scan_dtype, false) && fused_shape_ok(d, scan_dtype))) {
        set_error("%s: no scan of type %d for dtype %d, d %d", what, scan_dtype, exact_dtype, d);
        return SSS_EINVAL;
    }
    if (!c_scan || (reinterpret_cast<uintptr_t>(c_scan) & 15)) {
        set_error("%s: scan image (the %s) missing or not 16-byte aligned", what, format_of(scan_dtype)->name);
        return SSS_EINVAL;
    }
    if (scan_dtype == DT_F16 && (corpus_shift < -160 || corpus_shift > 160 || !(corpus_resid >= 0.f))) {
        set_error("%s: corpus_shift %d outside [-160, 160] or corpus_resid_norm %g not >= 0", what, corpus_shift, (double)corpus_resid);
        return SSS_EINVAL;
    }
    if (n >= (1L << 31) - 1024 || nq >= (1L << 31)) { set_error("%s: n and nq must be < 2^31", what); return SSS_EINVAL; }
    return SSS_OK;
}

ThrArgs thr_args(const void* q, const void* c_exact, int exact_dtype, int scan_dtype, int corpus_shift, float corpus_resid,
                 float corpus_max_norm, const int* qsel, long nsel, long n, int d, int k, int cap, long id_offset) {
    ThrArgs t = {};
    t.Q = q; t.C = c_exact; t.qsel = qsel; t.nsel = (int)nsel; t.d = d; t.dtype = exact_dtype; t.k = k; t.cap = cap; t.n = n;
    t.scan_dtype = scan_dtype; t.corpus_shift = corpus_shift; t.corpus_resid = corpus_resid; t.corpus_max_norm = corpus_max_norm;
    t.id_offset = id_offset;
    return t;
}

extern "C" size_t sss_ip_topk_state_bytes(int64_t nq) { return nq > 0 ? state_words(nq) * 4 : 0; }

extern "C" size_t sss_ip_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k, int dtype) {      // dtype: the C ABI's (0 / 1 / 4 / 6)
    if (nq <= 0 || n <= 0 || k <= 0 || !corpus_dtype_ok(dtype) || !fused_shape_ok(d, dtype)) return 0;
    return make_plan(nq, n, d, k, dtype).total_bytes;
}

static size_t ip_topk_scan_workspace_bytes(long nq, long n, int d, int k, int scan_dtype) {   // scan.h codes (0..4, 6)
    if (nq <= 0 || n <= 0 || k <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return make_plan(nq, n, d, k, scan_dtype).total_bytes;
}

extern "C" size_t sss_ip_topk_f16_workspace_bytes(int64_t nq, int64_t n, int d, int k) {
    return ip_topk_scan_workspace_bytes(nq, n, d, k, DT_F16);
}

extern "C" int sss_f16_shift(float amax) { return f16_shift(amax); }

// scan_dtype: what k_scan reads at c_scan (DT_F32 / DT_BF16 / DT_H16 / DT_I8: the corpus itself; DT_SPLIT: the
// [hi | lo] bf16 image of an f32 corpus; DT_F16: its scaled f16 image, corpus * 2^corpus_shift);
// c_exact / exact_dtype: the rows the candidates are re-scored from (and the element type of q).
static int ip_topk_impl(const char* what, const void* q, long nq, const void* c_scan, int scan_dtype, int corpus_shift,
                        float corpus_resid, const void* c_exact,
                        int exact_dtype, long n, int d, int k, long id_offset, float corpus_max_norm, float* D_out, long* I_out,
                        int* status, int* unproven_count, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                        hipStream_t st, const float* bias = nullptr, int d_row = 0) {
    // bias: the L2 search (sss_l2_topk below) -- the scan's keys are q.c + bias[row], the select's scores negated distances
    // d_row: elements of a stored row of c_exact where it is narrower than d, the width of q and c_scan (sss_pad_topk below); 0: d
    const bool l2 = bias != nullptr;
    if (nq <= 0 || n <= 0 || k <= 0) { set_error("%s: nq, n, k must be positive", what); return SSS_EINVAL; }
    int rc = check_scan_source(what, exact_dtype, scan_dtype, d, false, c_scan, corpus_shift, corpus_resid, n, nq);
    if (rc) return rc;
    if (k > 500) { set_error("%s: k too large (max 500)", what); return SSS_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(state) & 15)) {
        set_error("%s: workspace must be 256-byte aligned, state 16-byte aligned", what);
        return SSS_EINVAL;
    }
    if (!state || state_bytes < sss_ip_topk_state_bytes(nq)) { set_error("%s: state %zu < %zu bytes", what, state_bytes, sss_ip_topk_state_bytes(nq)); return SSS_EWORKSPACE; }
    const ScanPlan p = make_plan(nq, n, d, k, scan_dtype);
    if (ws_bytes < p.total_bytes) { set_error("%s: workspace %zu < %zu", what, ws_bytes, p.total_bytes); return SSS_EWORKSPACE; }
    char* w = reinterpret_cast<char*>(ws);

    ScanArgs a;
    a.Q = q; a.C = c_scan; a.nq = (int)nq; a.n = (int)n;
    a.tiles_per_split = p.tiles_per_split; a.total_tiles = p.total_tiles;
    a.S = p.S; a.G = p.G; a.J = p.J; a.Ju = p.Ju; a.cert = p.cert; a.boot = p.boot; a.append = p.append; a.cap = p.cap;
    a.tau_skip = p.tau_skip;
    unsigned* sw = reinterpret_cast<unsigned*>(state);
    a.slots = sw;
    a.cnt = sw + state_off_cnt(nq);
    a.maxlast = reinterpret_cast<unsigned long long*>(sw + state_off_maxlast(nq));
    a.cand = reinterpret_cast<unsigned long long*>(w);
    a.bias = bias; a.corpus_shift = corpus_shift;
    Prof& pr = g_prof[current_device()];
    const bool prof = pr.on && pr.n < PROF_RING;
    if (prof) (void)hipEventRecord(pr.ev[2 * pr.n], st);
    rc = launch_scan(scan_dtype, d, p.tile_rows, a, st);
    if (prof) { (void)hipEventRecord(pr.ev[2 * pr.n + 1], st); ++pr.n; }
    if (rc) return rc;                 // nothing ran: the state is still clean

    SelectArgs s;
    s.Q = q; s.C = c_exact; s.nq = (int)nq; s.d = d; s.dtype = exact_dtype; s.scan_dtype = scan_dtype; s.corpus_shift = corpus_shift; s.corpus_resid = corpus_resid;
    s.k = k; s.K2 = p.K2; s.J = p.J; s.cap = p.cap; s.tau_skip = p.tau_skip;
    s.cand = a.cand; s.slots = a.slots; s.cnt = a.cnt; s.maxlast = a.maxlast;
    s.id_offset = id_offset; s.corpus_max_norm = corpus_max_norm;
    s.D_out = D_out; s.I_out = I_out; s.status = status; s.unproven_count = unproven_count;
    s.metric = l2 ? 1 : 0;
    s.d_row = d_row;
    rc = launch_select(s, st);
    if (rc) (void)hipMemsetAsync(state, 0, sss_ip_topk_state_bytes(nq), st);   // the scan dirtied it and nobody will clear it
    return rc;
}

// Threshold form of k_scan (sss_ip_topk_threshold, sss_range_search_count): `prepare` writes the thresholds t.thr and
// zeroes the counters t.cnt of the t.nsel queries t.qsel, the scan keeps every row above its query's threshold in
// t.cand, `select` re-scores them.
template <class Prepare, class Select>
static int run_threshold_form(const ThrArgs& t, const void* c_scan, const ScanPlan& p, Prepare prepare, Select select, hipStream_t st,
                              const float* bias = nullptr) {
    int rc = prepare();
    if (rc) return rc;
    ScanArgs a = {};
    a.Q = t.Q; a.C = c_scan; a.nq = t.nsel; a.n = (int)t.n;
    a.tiles_per_split = p.tiles_per_split; a.total_tiles = p.total_tiles;
    a.S = p.S; a.G = p.G; a.J = 0; a.Ju = 0; a.cert = 1; a.boot = 0; a.append = 0; a.cap = p.cap;
    a.slots = nullptr; a.cnt = t.cnt; a.maxlast = nullptr;
    a.cand = const_cast<unsigned long long*>(t.cand);
    a.qsel = t.qsel; a.thr = t.thr;
    a.bias = bias; a.corpus_shift = t.corpus_shift;
    rc = launch_scan(t.scan_dtype, t.d, p.tile_rows, a, st);
    if (rc) return rc;
    return select();
}

// Threshold rung for the queries `qsel` a fused search left unproven (select_thr.hip: THRESHOLD RUNG).
// Workspace: thr f32 [nsel] | cnt u32 [nsel] | (256-byte aligned) cand u64 [nsel][cap].
constexpr int THR_CAP = 8192;       // rows kept per query (64 KB of keys in LDS for the sort)
static size_t thr_head_bytes(long nsel) { return ((size_t)nsel * 8 + 255) & ~(size_t)255; }

extern "C" size_t sss_ip_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d, int scan_dtype) {
    if (nsel <= 0 || n <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return thr_head_bytes(nsel) + make_thr_plan(nsel, n, d, scan_dtype, THR_CAP).total_bytes;
}

static int topk_threshold_impl(const char* what, const void* q, const int* qsel, long nsel, const void* c_exact, int exact_dtype,
                               const void* c_scan, int scan_dtype, int corpus_shift, float corpus_resid, long n, int d, int k,
                               long id_offset, float corpus_max_norm, float* D_out, long* I_out, int* status, void* ws, size_t ws_bytes,
                               hipStream_t st, const float* bias = nullptr, int d_row = 0) {
    if (nsel <= 0 || n <= 0 || k <= 0 || !qsel) { set_error("%s: nsel, n, k must be positive", what); return SSS_EINVAL; }
    const int rc = check_scan_source(what, exact_dtype, scan_dtype, d, false, c_scan, corpus_shift, corpus_resid, n, nsel);
    if (rc) return rc;
    if (k > THR_CAP) { set_error("%s: k too large (max %d)", what, THR_CAP); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(ws) & 255) { set_error("%s: workspace must be 256-byte aligned", what); return SSS_EINVAL; }
    const ScanPlan p = make_thr_plan(nsel, n, d, scan_dtype, THR_CAP);
    if (ws_bytes < thr_head_bytes(nsel) + p.total_bytes) { set_error("%s: workspace %zu < %zu", what, ws_bytes, thr_head_bytes(nsel) + p.total_bytes); return SSS_EWORKSPACE; }
    char* w = reinterpret_cast<char*>(ws);
    ThrArgs t = thr_args(q, c_exact, exact_dtype, scan_dtype, corpus_shift, corpus_resid, corpus_max_norm, qsel, nsel, n, d, k, p.cap,
                         id_offset);
    t.thr = reinterpret_cast<float*>(w);
    t.cnt = reinterpret_cast<unsigned*>(w + (size_t)nsel * 4);
    t.cand = reinterpret_cast<unsigned long long*>(w + thr_head_bytes(nsel));
    t.D_out = D_out; t.I_out = I_out; t.status = status;
    t.metric = bias != nullptr ? 1 : 0;
    t.d_row = d_row;                    // (sss_pad_topk_threshold; 0: the stored rows are d wide)
    return run_threshold_form(t, c_scan, p, [&] { return launch_thr_prepare(t, st); }, [&] { return launch_select_all(t, st); }, st, bias);
}

extern "C" int sss_ip_topk_threshold(const void* q, const int32_t* qsel, int64_t nsel, const void* corpus, int dtype,
                                     const void* scan_image, int scan_dtype, int corpus_shift, float corpus_resid_norm, int64_t n, int d,
                                     int k, int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return topk_threshold_impl("ip_topk_threshold", q, qsel, nsel, corpus, dtype, scan_image, scan_dtype, corpus_shift, corpus_resid_norm, n, d,
                               k, id_offset, corpus_max_norm, D_out, I_out, status, workspace, workspace_bytes, st);
}

// RANGE SEARCH, fused route (select_thr.hip: RANGE SEARCH): the threshold rung's scan with thresholds from per-query radii.
// Workspace: thr f32 [nq] | cnt u32 [nq] | (256-byte aligned) qsel i32 [nq] | (256-byte aligned) cand u64 [nq][THR_CAP].
// sss_range_search_count leaves each resolved query's entries in its candidate row; sss_range_search_fill copies them out.
static size_t range_head_bytes(long nq) { return thr_head_bytes(nq) + (((size_t)nq * 4 + 255) & ~(size_t)255); }
static size_t range_cand_bytes(long nq) { return ((size_t)nq * THR_CAP * 8 + 255) & ~(size_t)255; }

extern "C" size_t sss_range_search_workspace_bytes(int64_t nq, int64_t n, int d, int scan_dtype) {
    if (nq <= 0 || n <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return range_head_bytes(nq) + make_thr_plan(nq, n, d, scan_dtype, THR_CAP).total_bytes;
}

extern "C" int sss_range_search_count(const void* q, int64_t nq, const void* corpus, int dtype, const void* scan_image, int scan_dtype,
                                      int corpus_shift, float corpus_resid_norm, int64_t n, int d, const float* radius,
                                      float corpus_max_norm, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || n <= 0) { set_error("range_search_count: nq, n must be positive"); return SSS_EINVAL; }
    const int rc = check_scan_source("range_search_count", dtype, scan_dtype, d, false, scan_image, corpus_shift, corpus_resid_norm, n, nq);
    if (rc) return rc;
    if (!q || !corpus || !radius || !counts || !status) { set_error("range_search_count: q, corpus, radius, counts and status are required"); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("range_search_count: workspace must be 256-byte aligned"); return SSS_EINVAL; }
    const ScanPlan p = make_thr_plan(nq, n, d, scan_dtype, THR_CAP);
    const size_t need = range_head_bytes(nq) + p.total_bytes;
    if (!workspace || workspace_bytes < need) { set_error("range_search_count: workspace %zu < %zu", workspace_bytes, need); return SSS_EWORKSPACE; }
    char* w = reinterpret_cast<char*>(workspace);
    int* qsel = reinterpret_cast<int*>(w + thr_head_bytes(nq));
    ThrArgs t = thr_args(q, corpus, dtype, scan_dtype, corpus_shift, corpus_resid_norm, corpus_max_norm, qsel, nq, n, d, 1, p.cap, 0);
    t.thr = reinterpret_cast<float*>(w);
    t.cnt = reinterpret_cast<unsigned*>(w + (size_t)nq * 4);
    t.cand = reinterpret_cast<unsigned long long*>(w + range_head_bytes(nq));
    return run_threshold_form(t, scan_image, p, [&] { return launch_range_prepare(t, radius, qsel, st); },
                              [&] { return launch_range_select(t, radius, counts, status, st); }, st);
}

extern "C" int sss_range_search_fill(int64_t nq, const int64_t* lims, int64_t id_offset, float* D_out, int64_t* I_out,
                                     const void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || nq >= (1L << 31)) { set_error("range_search_fill: nq must be in [1, 2^31)"); return SSS_EINVAL; }
    if (!lims) { set_error("range_search_fill: lims is required"); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("range_search_fill: workspace must be 256-byte aligned"); return SSS_EINVAL; }
    const size_t need = range_head_bytes(nq) + range_cand_bytes(nq);
    if (!workspace || workspace_bytes < need) { set_error("range_search_fill: workspace %zu < %zu", workspace_bytes, need); return SSS_EWORKSPACE; }
    const char* w = reinterpret_cast<const char*>(workspace);
    return launch_range_fill(reinterpret_cast<const unsigned*>(w + (size_t)nq * 4),
                             reinterpret_cast<const unsigned long long*>(w + range_head_bytes(nq)), THR_CAP, nq, lims, id_offset, D_out,
                             I_out, st);
}

extern "C" int sss_ip_topk(const void* q, int64_t nq, const void* corpus, int64_t n, int d, int k, int dtype, int64_t id_offset,
                           float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                           size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return ip_topk_impl("ip_topk", q, nq, corpus, dtype, 0, 0.f, corpus, dtype, n, d, k, id_offset, corpus_max_norm, D_out, I_out, status,
                        unproven_count, state, state_bytes, workspace, workspace_bytes, st);
}

extern "C" int sss_ip_topk_split(const float* q, int64_t nq, const float* corpus, const uint16_t* scan_image, int64_t n, int d, int k,
                                 int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                 int32_t* unproven_count, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return ip_topk_impl("ip_topk_split", q, nq, scan_image, DT_SPLIT, 0, 0.f, corpus, DT_F32, n, d, k, id_offset, corpus_max_norm, D_out,
                        I_out, status, unproven_count, state, state_bytes, workspace, workspace_bytes, st);
}

extern "C" int sss_ip_topk_f16(const float* q, int64_t nq, const float* corpus, const uint16_t* scan_image, int corpus_shift,
                               float corpus_resid_norm, int64_t n, int d, int k, int64_t id_offset, float corpus_max_norm, float* D_out,
                               int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state, size_t state_bytes,
                               void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    return ip_topk_impl("ip_topk_f16", q, nq, scan_image, DT_F16, corpus_shift, corpus_resid_norm, corpus, DT_F32, n, d, k, id_offset, corpus_max_norm,
                        D_out, I_out, status, unproven_count, state, state_bytes, workspace, workspace_bytes, st);
}

// ------------------------------------------------------------------------------------------
// L2 top-k on the same scans (include/sss_l2.h): float32 rows, the scan's keys biased by bias[row] = -|c_row|^2 / 2
// (rowops.hip: sss_l2_row_bias), scores the negated canonical squared distances (select_dev.h: err_bound_l2, DT_F32_L2).
static int check_l2(const char* what, int scan_dtype, const float* q, const float* c, const float* bias, const float* D_out,
                    const long* I_out, const int* status) {
    if (scan_dtype != DT_F32 && scan_dtype != DT_SPLIT && scan_dtype != DT_F16) {
        set_error("%s: scan_dtype %d is not a scan of float32 rows (0 the rows, 2 the split image, 3 the f16 image)", what, scan_dtype);
        return SSS_EINVAL;
    }
    if (!bias || (reinterpret_cast<uintptr_t>(bias) & 15)) { set_error("%s: row bias missing or not 16-byte aligned", what); return SSS_EINVAL; }
    if (!q || !c || !D_out || !I_out || !status) { set_error("%s: q, corpus, D_out, I_out and status are required", what); return SSS_EINVAL; }
    return SSS_OK;
}

extern "C" size_t sss_l2_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k, int scan_dtype) {
    if (scan_dtype != DT_F32 && scan_dtype != DT_SPLIT && scan_dtype != DT_F16) return 0;
    return ip_topk_scan_workspace_bytes(nq, n, d, k, scan_dtype);
}

extern "C" int sss_l2_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                           float corpus_resid_norm, const float* bias, int64_t n, int d, int k, int64_t id_offset,
                           float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                           size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || n <= 0 || k <= 0) { set_error("l2_topk: nq, n, k must be positive"); return SSS_EINVAL; }
    int rc = check_scan_source("l2_topk", DT_F32, scan_dtype, d, false, scan_image, corpus_shift, corpus_resid_norm, n, nq);
    if (!rc) rc = check_l2("l2_topk", scan_dtype, q, corpus, bias, D_out, I_out, status);
    if (rc) return rc;
    return ip_topk_impl("l2_topk", q, nq, scan_image, scan_dtype, corpus_shift, corpus_resid_norm, corpus, DT_F32, n, d, k, id_offset, corpus_max_norm,
                        D_out, I_out, status, unproven_count, state, state_bytes, workspace, workspace_bytes, st, bias);
}

extern "C" size_t sss_l2_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d, int scan_dtype) {
    if (scan_dtype != DT_F32 && scan_dtype != DT_SPLIT && scan_dtype != DT_F16) return 0;
    return sss_ip_topk_threshold_workspace_bytes(nsel, n, d, scan_dtype);
}

extern "C" int sss_l2_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                                     int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n, int d,
                                     int k, int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nsel <= 0 || n <= 0 || k <= 0 || !qsel) { set_error("l2_topk_threshold: nsel, n, k must be positive"); return SSS_EINVAL; }
    int rc = check_scan_source("l2_topk_threshold", DT_F32, scan_dtype, d, false, scan_image, corpus_shift, corpus_resid_norm, n, nsel);
    if (!rc) rc = check_l2("l2_topk_threshold", scan_dtype, q, corpus, bias, D_out, I_out, status);
    if (rc) return rc;
    if (!workspace) { set_error("l2_topk_threshold: workspace 0 < %zu", sss_l2_topk_threshold_workspace_bytes(nsel, n, d, scan_dtype)); return SSS_EWORKSPACE; }
    return topk_threshold_impl("l2_topk_threshold", q, qsel, nsel, corpus, DT_F32, scan_image, scan_dtype, corpus_shift, corpus_resid_norm, n, d, k,
                               id_offset, corpus_max_norm, D_out, I_out, status, workspace, workspace_bytes, st, bias);
}

// ------------------------------------------------------------------------------------------
// Scans at a width the row does not have (include/sss_pad.h): float32 rows of d_row elements, q and c_scan zero-extended to
// d_scan -- a width of scan_dtype's fused kernels -- by the builders of rowops.hip.  Zero columns add nothing to a dot
// product or to |c|^2, so the scan, its keys and its bound (for a chain of d_scan terms: what the scan really summed) are
// those of a d_scan-wide corpus; the select kernels re-score from the d_row-wide rows (SelectArgs::d_row).
static int check_pad(const char* what, int scan_dtype, int d_row, int d_scan) {
    if (d_row <= 0 || d_row % 4 || d_row > d_scan) {
        set_error("%s: need 0 < d_row <= d_scan and d_row %% 4 == 0 (d_row %d, d_scan %d)", what, d_row, d_scan);
        return SSS_EINVAL;
    }
    if (scan_dtype != DT_F32 && scan_dtype != DT_SPLIT && scan_dtype != DT_F16) {
        set_error("%s: scan_dtype %d is not a scan of float32 rows (0 the padded rows, 2 the split image, 3 the f16 image)", what, scan_dtype);
        return SSS_EINVAL;
    }
    return SSS_OK;
}
static bool pad_shape_ok(int d_row, int d_scan, int scan_dtype) {
    return d_row > 0 && d_row % 4 == 0 && d_row <= d_scan && (scan_dtype == DT_F32 || scan_dtype == DT_SPLIT || scan_dtype == DT_F16) &&
           fused_shape_ok(d_scan, scan_dtype);
}
static int check_pad_buffers(const char* what, const float* q, const float* c, const float* bias, const float* D_out, const long* I_out,
                             const int* status) {
    if (bias && (reinterpret_cast<uintptr_t>(bias) & 15)) { set_error("%s: row bias not 16-byte aligned", what); return SSS_EINVAL; }
    if (!q || !c || !D_out || !I_out || !status) { set_error("%s: q, corpus, D_out, I_out and status are required", what); return SSS_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(q) & 15) || (reinterpret_cast<uintptr_t>(c) & 15)) { set_error("%s: q and corpus must be 16-byte aligned", what); return SSS_EINVAL; }
    return SSS_OK;
}

extern "C" size_t sss_pad_topk_workspace_bytes(int64_t nq, int64_t n, int d_row, int d_scan, int k, int scan_dtype) {
    if (!pad_shape_ok(d_row, d_scan, scan_dtype)) return 0;
    return ip_topk_scan_workspace_bytes(nq, n, d_scan, k, scan_dtype);
}

extern "C" int sss_pad_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                            float corpus_resid_norm, const float* bias, int64_t n, int d_row, int d_scan, int k, int64_t id_offset,
                            float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                            size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || n <= 0 || k <= 0) { set_error("pad_topk: nq, n, k must be positive"); return SSS_EINVAL; }
    int rc = check_pad("pad_topk", scan_dtype, d_row, d_scan);
    if (!rc) rc = check_scan_source("pad_topk", DT_F32, scan_dtype, d_scan, false, scan_image, corpus_shift, corpus_resid_norm, n, nq);
    if (!rc) rc = check_pad_buffers("pad_topk", q, corpus, bias, D_out, I_out, status);
    if (rc) return rc;
    if (!workspace) { set_error("pad_topk: workspace 0 < %zu", sss_pad_topk_workspace_bytes(nq, n, d_row, d_scan, k, scan_dtype)); return SSS_EWORKSPACE; }
    return ip_topk_impl("pad_topk", q, nq, scan_image, scan_dtype, corpus_shift, corpus_resid_norm, corpus, DT_F32, n, d_scan, k, id_offset, corpus_max_norm,
                        D_out, I_out, status, unproven_count, state, state_bytes, workspace, workspace_bytes, st, bias, d_row);
}

extern "C" size_t sss_pad_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d_row, int d_scan, int scan_dtype) {
    if (!pad_shape_ok(d_row, d_scan, scan_dtype)) return 0;
    return sss_ip_topk_threshold_workspace_bytes(nsel, n, d_scan, scan_dtype);
}

extern "C" int sss_pad_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                                      int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n,
                                      int d_row, int d_scan, int k, int64_t id_offset, float corpus_max_norm, float* D_out,
                                      int64_t* I_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nsel <= 0 || n <= 0 || k <= 0 || !qsel) { set_error("pad_topk_threshold: nsel, n, k must be positive"); return SSS_EINVAL; }
    int rc = check_pad("pad_topk_threshold", scan_dtype, d_row, d_scan);
    if (!rc) rc = check_scan_source("pad_topk_threshold", DT_F32, scan_dtype, d_scan, false, scan_image, corpus_shift, corpus_resid_norm, n, nsel);
    if (!rc) rc = check_pad_buffers("pad_topk_threshold", q, corpus, bias, D_out, I_out, status);
    if (rc) return rc;
    if (!workspace) { set_error("pad_topk_threshold: workspace 0 < %zu", sss_pad_topk_threshold_workspace_bytes(nsel, n, d_row, d_scan, scan_dtype)); return SSS_EWORKSPACE; }
    return topk_threshold_impl("pad_topk_threshold", q, qsel, nsel, corpus, DT_F32, scan_image, scan_dtype, corpus_shift, corpus_resid_norm, n, d_scan, k,
                               id_offset, corpus_max_norm, D_out, I_out, status, workspace, workspace_bytes, st, bias, d_row);
}

}  // namespace sss
