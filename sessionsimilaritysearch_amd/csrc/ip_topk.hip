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

// the scans an L2 or padded search may name: the float32 rows themselves or one of their two images
static bool scans_f32_rows(int scan_dtype) { return scan_dtype == DT_F32 || scan_dtype == DT_SPLIT || scan_dtype == DT_F16; }
static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// c.scan_dtype: what k_scan reads for rows of c.exact_dtype (elem.h: scan_pair_ok).
int check_scan_source(const SearchCall& c, bool long_rows) {
    if (long_rows && c.exact_dtype == DT_I8) { set_error("%s: int8 rows (dtype %d) have no long-row scan: d in {256,512,1024} on the fused scan, else the exhaustive kernels", c.what, DT_I8); return SSS_EINVAL; }
    if (!(long_rows ? long_shape_ok(c.d, c.exact_dtype, c.scan_dtype)
                    : scan_pair_ok(c.exact_dtype, c.scan_dtype, false) && fused_shape_ok(c.d, c.scan_dtype))) { set_error("%s: no scan of type %d for dtype %d, d %d", c.what, c.scan_dtype, c.exact_dtype, c.d); return SSS_EINVAL; }
    if (!c.c_scan || misaligned16(c.c_scan)) { set_error("%s: scan image (the %s) missing or not 16-byte aligned", c.what, format_of(c.scan_dtype)->name); return SSS_EINVAL; }
    if (c.scan_dtype == DT_F16 && (c.corpus_shift < -160 || c.corpus_shift > 160 || !(c.corpus_resid >= 0.f))) { set_error("%s: corpus_shift %d outside [-160, 160] or corpus_resid_norm %g not >= 0", c.what, c.corpus_shift, (double)c.corpus_resid); return SSS_EINVAL; }
    if (c.n >= (1L << 31) - 1024 || c.nq >= (1L << 31)) { set_error("%s: n and nq must be < 2^31", c.what); return SSS_EINVAL; }
    return SSS_OK;
}

int check_buffers(const SearchCall& c, bool bias_required, bool aligned_rows) {
    if (bias_required ? !c.bias || misaligned16(c.bias) : c.bias && misaligned16(c.bias)) { set_error(bias_required ? "%s: row bias missing or not 16-byte aligned" : "%s: row bias not 16-byte aligned", c.what); return SSS_EINVAL; }
    if (!c.q || !c.c_exact || !c.D_out || !c.I_out || !c.status) { set_error("%s: q, corpus, D_out, I_out and status are required", c.what); return SSS_EINVAL; }
    if (aligned_rows && (misaligned16(c.q) || misaligned16(c.c_exact))) { set_error("%s: q and corpus must be 16-byte aligned", c.what); return SSS_EINVAL; }
    return SSS_OK;
}

// What a fused search checks between its counts and its k, in the order each family has always checked it (and the tests of
// each pin): the pad family looks at its two widths and its scan type BEFORE the scan source and wants q and corpus aligned;
// the L2 family requires the bias.  (An L2 call's scan type needs no look of its own: float32 rows pair with nothing else.)
static int check_source_and_buffers(const SearchCall& c) {
    if (c.family == FAM_PAD) {
        if (c.d_row <= 0 || c.d_row % 4 || c.d_row > c.d) { set_error("%s: need 0 < d_row <= d_scan and d_row %% 4 == 0 (d_row %d, d_scan %d)", c.what, c.d_row, c.d); return SSS_EINVAL; }
        if (!scans_f32_rows(c.scan_dtype)) { set_error("%s: scan_dtype %d is not a scan of float32 rows (0 the padded rows, 2 the split image, 3 the f16 image)", c.what, c.scan_dtype); return SSS_EINVAL; }
    }
    int rc = check_scan_source(c, false);
    if (!rc && c.family != FAM_IP) rc = check_buffers(c, c.family == FAM_L2, c.family == FAM_PAD);
    return rc;
}

ThrArgs thr_args(const SearchCall& c, int cap) {
    ThrArgs t = {};
    t.Q = c.q; t.C = c.c_exact; t.qsel = c.qsel; t.nsel = (int)c.nq; t.d = c.d; t.dtype = c.exact_dtype; t.k = c.k; t.cap = cap; t.n = c.n;
    t.scan_dtype = c.scan_dtype; t.corpus_shift = c.corpus_shift; t.corpus_resid = c.corpus_resid; t.corpus_max_norm = c.corpus_max_norm;
    t.id_offset = c.id_offset; t.D_out = c.D_out; t.I_out = c.I_out; t.status = c.status;
    t.metric = c.bias != nullptr ? 1 : 0; t.d_row = c.d_row;
    return t;
}

// The ScanArgs a plan and a call determine; the caller adds the arrays the scan writes.
static ScanArgs scan_args(const ScanPlan& p, const SearchCall& c) {
    ScanArgs a = {};
    a.Q = c.q; a.C = c.c_scan; a.nq = (int)c.nq; a.n = (int)c.n;
    a.tiles_per_split = p.tiles_per_split; a.total_tiles = p.total_tiles; a.tau_skip = p.tau_skip;
    a.S = p.S; a.G = p.G; a.J = p.J; a.Ju = p.Ju; a.cert = p.cert; a.boot = p.boot; a.append = p.append; a.cap = p.cap;
    a.bias = c.bias; a.corpus_shift = c.corpus_shift;
    return a;
}

extern "C" size_t sss_ip_topk_state_bytes(int64_t nq) { return nq > 0 ? state_words(nq) * 4 : 0; }

static size_t ip_topk_scan_workspace_bytes(long nq, long n, int d, int k, int scan_dtype) {   // scan.h codes (0..4, 6)
    if (nq <= 0 || n <= 0 || k <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return make_plan(nq, n, d, k, scan_dtype).total_bytes;
}

extern "C" size_t sss_ip_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k, int dtype) {      // dtype: the C ABI's (0 / 1 / 4 / 6)
    return corpus_dtype_ok(dtype) ? ip_topk_scan_workspace_bytes(nq, n, d, k, dtype) : 0;
}

extern "C" size_t sss_ip_topk_f16_workspace_bytes(int64_t nq, int64_t n, int d, int k) { return ip_topk_scan_workspace_bytes(nq, n, d, k, DT_F16); }

extern "C" int sss_f16_shift(float amax) { return f16_shift(amax); }

// The fused search of every family: c.scan_dtype is what k_scan reads at c.c_scan (DT_F32 / DT_BF16 / DT_H16 / DT_I8: the
// corpus itself; DT_SPLIT: the [hi | lo] bf16 image of an f32 corpus; DT_F16: its scaled f16 image, corpus * 2^corpus_shift);
// c.c_exact / c.exact_dtype: the rows the candidates are re-scored from (and the element type of q).
static int ip_topk_impl(const SearchCall& c) {
    if (c.nq <= 0 || c.n <= 0 || c.k <= 0) { set_error("%s: nq, n, k must be positive", c.what); return SSS_EINVAL; }
    int rc = check_source_and_buffers(c);
    if (rc) return rc;
    // (the pad family alone turns a null workspace away, and does so before it looks at k)
    if (c.family == FAM_PAD && !c.ws) { set_error("%s: workspace 0 < %zu", c.what, make_plan(c.nq, c.n, c.d, c.k, c.scan_dtype).total_bytes); return SSS_EWORKSPACE; }
    if (c.k > 500) { set_error("%s: k too large (max 500)", c.what); return SSS_EINVAL; }
    if ((reinterpret_cast<uintptr_t>(c.ws) & 255) || misaligned16(c.state)) { set_error("%s: workspace must be 256-byte aligned, state 16-byte aligned", c.what); return SSS_EINVAL; }
    const size_t state_need = sss_ip_topk_state_bytes(c.nq);
    if (!c.state || c.state_bytes < state_need) { set_error("%s: state %zu < %zu bytes", c.what, c.state_bytes, state_need); return SSS_EWORKSPACE; }
    const ScanPlan p = make_plan(c.nq, c.n, c.d, c.k, c.scan_dtype);       // workspace: cand u64 [nq][cap], nothing else
    if (c.ws_bytes < p.total_bytes) { set_error("%s: workspace %zu < %zu", c.what, c.ws_bytes, p.total_bytes); return SSS_EWORKSPACE; }

    ScanArgs a = scan_args(p, c);
    unsigned* sw = reinterpret_cast<unsigned*>(c.state);
    a.slots = sw;
    a.cnt = sw + state_off_cnt(c.nq);
    a.maxlast = reinterpret_cast<unsigned long long*>(sw + state_off_maxlast(c.nq));
    a.cand = reinterpret_cast<unsigned long long*>(c.ws);
    Prof& pr = g_prof[current_device()];
    const bool prof = pr.on && pr.n < PROF_RING;
    if (prof) (void)hipEventRecord(pr.ev[2 * pr.n], c.st);
    rc = launch_scan(c.scan_dtype, c.d, p.tile_rows, a, c.st);
    if (prof) { (void)hipEventRecord(pr.ev[2 * pr.n + 1], c.st); ++pr.n; }
    if (rc) return rc;                 // nothing ran: the state is still clean

    SelectArgs s;
    s.Q = c.q; s.C = c.c_exact; s.nq = (int)c.nq; s.d = c.d; s.dtype = c.exact_dtype;
    s.scan_dtype = c.scan_dtype; s.corpus_shift = c.corpus_shift; s.corpus_resid = c.corpus_resid;
    s.k = c.k; s.K2 = p.K2; s.J = p.J; s.cap = p.cap; s.tau_skip = p.tau_skip;
    s.cand = a.cand; s.slots = a.slots; s.cnt = a.cnt; s.maxlast = a.maxlast;
    s.id_offset = c.id_offset; s.corpus_max_norm = c.corpus_max_norm;
    s.D_out = c.D_out; s.I_out = c.I_out; s.status = c.status; s.unproven_count = c.unproven_count;
    s.metric = c.bias != nullptr ? 1 : 0; s.d_row = c.d_row;
    rc = launch_select(s, c.st);
    if (rc) (void)hipMemsetAsync(c.state, 0, state_need, c.st);   // the scan dirtied it and nobody will clear it
    return rc;
}

// Threshold form of k_scan (sss_ip_topk_threshold, sss_range_search_count): `prepare` writes the thresholds t.thr and
// zeroes the counters t.cnt of the t.nsel queries t.qsel, the scan keeps every row above its query's threshold in
// t.cand, `select` re-scores them.
template <class Prepare, class Select>
static int run_threshold_form(const SearchCall& c, const ThrArgs& t, const ScanPlan& p, Prepare prepare, Select select) {
    int rc = prepare();
    if (rc) return rc;
    ScanArgs a = scan_args(p, c);
    a.J = 0; a.Ju = 0; a.cert = 1; a.boot = 0; a.append = 0;        // no slots, no bootstrap: the thresholds are given
    a.slots = nullptr; a.cnt = t.cnt; a.maxlast = nullptr;
    a.cand = const_cast<unsigned long long*>(t.cand);
    a.qsel = t.qsel; a.thr = t.thr;
    rc = launch_scan(c.scan_dtype, c.d, p.tile_rows, a, c.st);
    if (rc) return rc;
    return select();
}

// Workspace of the threshold form, written ONCE (offsets in bytes; the sizing functions return `total`, the searches read
// their pointers from it).  Threshold rung for the queries `qsel` a fused search left unproven (select_thr.hip: THRESHOLD
// RUNG): thr f32 [nsel] | cnt u32 [nsel] | (256-byte aligned) cand u64 [nsel][cap].  RANGE SEARCH, fused route
// (select_thr.hip: RANGE SEARCH; with_qsel): its identity selection qsel i32 [nq], 256-byte aligned, between cnt and cand.
constexpr int THR_CAP = 8192;       // rows kept per query (64 KB of keys in LDS for the sort)
struct ThrLayout { size_t thr, cnt, qsel, cand, total; };
static ThrLayout thr_layout(long nsel, bool with_qsel, size_t cand_bytes) {
    ThrLayout l;
    l.thr = 0; l.cnt = (size_t)nsel * 4; l.qsel = al256((size_t)nsel * 8);
    l.cand = l.qsel + (with_qsel ? al256((size_t)nsel * 4) : 0); l.total = l.cand + cand_bytes;
    return l;
}
static void carve(ThrArgs& t, void* ws, const ThrLayout& l) {
    char* w = reinterpret_cast<char*>(ws);
    t.thr = reinterpret_cast<float*>(w + l.thr);
    t.cnt = reinterpret_cast<unsigned*>(w + l.cnt);
    t.cand = reinterpret_cast<unsigned long long*>(w + l.cand);
}

extern "C" size_t sss_ip_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d, int scan_dtype) {
    if (nsel <= 0 || n <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return thr_layout(nsel, false, make_thr_plan(nsel, n, d, scan_dtype, THR_CAP).total_bytes).total;
}

static int topk_threshold_impl(const SearchCall& c) {
    if (c.nq <= 0 || c.n <= 0 || c.k <= 0 || !c.qsel) { set_error("%s: nsel, n, k must be positive", c.what); return SSS_EINVAL; }
    const int rc = check_source_and_buffers(c);
    if (rc) return rc;
    const ScanPlan p = make_thr_plan(c.nq, c.n, c.d, c.scan_dtype, THR_CAP);
    const ThrLayout l = thr_layout(c.nq, false, p.total_bytes);
    // (the L2 and pad families turn a null workspace away, and do so before they look at k)
    if (c.family != FAM_IP && !c.ws) { set_error("%s: workspace 0 < %zu", c.what, l.total); return SSS_EWORKSPACE; }
    if (c.k > THR_CAP) { set_error("%s: k too large (max %d)", c.what, THR_CAP); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(c.ws) & 255) { set_error("%s: workspace must be 256-byte aligned", c.what); return SSS_EINVAL; }
    if (c.ws_bytes < l.total) { set_error("%s: workspace %zu < %zu", c.what, c.ws_bytes, l.total); return SSS_EWORKSPACE; }
    ThrArgs t = thr_args(c, p.cap);
    carve(t, c.ws, l);
    return run_threshold_form(c, t, p, [&] { return launch_thr_prepare(t, c.st); }, [&] { return launch_select_all(t, c.st); });
}

extern "C" int sss_ip_topk_threshold(const void* q, const int32_t* qsel, int64_t nsel, const void* corpus, int dtype,
                                     const void* scan_image, int scan_dtype, int corpus_shift, float corpus_resid_norm, int64_t n, int d,
                                     int k, int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return topk_threshold_impl({.what = "ip_topk_threshold", .family = FAM_IP, .q = q, .nq = nsel, .qsel = qsel, .c_exact = corpus, .exact_dtype = dtype,
                                .c_scan = scan_image, .scan_dtype = scan_dtype, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .n = n, .d = d, .k = k,
                                .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status, .ws = workspace,
                                .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

extern "C" size_t sss_range_search_workspace_bytes(int64_t nq, int64_t n, int d, int scan_dtype) {
    if (nq <= 0 || n <= 0 || !fused_shape_ok(d, scan_dtype)) return 0;
    return thr_layout(nq, true, make_thr_plan(nq, n, d, scan_dtype, THR_CAP).total_bytes).total;
}

// sss_range_search_count leaves each resolved query's entries in its candidate row; sss_range_search_fill copies them out.
// (status is not part of the record: the range kernels take it beside their ThrArgs, whose own status stays null)
extern "C" int sss_range_search_count(const void* q, int64_t nq, const void* corpus, int dtype, const void* scan_image, int scan_dtype,
                                      int corpus_shift, float corpus_resid_norm, int64_t n, int d, const float* radius,
                                      float corpus_max_norm, int64_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    SearchCall c = {.what = "range_search_count", .family = FAM_IP, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = dtype, .c_scan = scan_image,
                    .scan_dtype = scan_dtype, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .n = n, .d = d, .k = 1, .corpus_max_norm = corpus_max_norm,
                    .ws = workspace, .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)};
    if (c.nq <= 0 || c.n <= 0) { set_error("%s: nq, n must be positive", c.what); return SSS_EINVAL; }
    const int rc = check_scan_source(c, false);
    if (rc) return rc;
    if (!q || !corpus || !radius || !counts || !status) { set_error("%s: q, corpus, radius, counts and status are required", c.what); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(c.ws) & 255) { set_error("%s: workspace must be 256-byte aligned", c.what); return SSS_EINVAL; }
    const ScanPlan p = make_thr_plan(c.nq, c.n, c.d, c.scan_dtype, THR_CAP);
    const ThrLayout l = thr_layout(c.nq, true, p.total_bytes);
    if (!c.ws || c.ws_bytes < l.total) { set_error("%s: workspace %zu < %zu", c.what, c.ws_bytes, l.total); return SSS_EWORKSPACE; }
    int* qsel = reinterpret_cast<int*>(reinterpret_cast<char*>(c.ws) + l.qsel);
    c.qsel = qsel;
    ThrArgs t = thr_args(c, p.cap);
    carve(t, c.ws, l);
    return run_threshold_form(c, t, p, [&] { return launch_range_prepare(t, radius, qsel, c.st); },
                              [&] { return launch_range_select(t, radius, counts, status, c.st); });
}

extern "C" int sss_range_search_fill(int64_t nq, const int64_t* lims, int64_t id_offset, float* D_out, int64_t* I_out,
                                     const void* workspace, size_t workspace_bytes, void* stream) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (nq <= 0 || nq >= (1L << 31)) { set_error("range_search_fill: nq must be in [1, 2^31)"); return SSS_EINVAL; }
    if (!lims) { set_error("range_search_fill: lims is required"); return SSS_EINVAL; }
    if (reinterpret_cast<uintptr_t>(workspace) & 255) { set_error("range_search_fill: workspace must be 256-byte aligned"); return SSS_EINVAL; }
    const ThrLayout l = thr_layout(nq, true, al256((size_t)nq * THR_CAP * 8));
    if (!workspace || workspace_bytes < l.total) { set_error("range_search_fill: workspace %zu < %zu", workspace_bytes, l.total); return SSS_EWORKSPACE; }
    const char* w = reinterpret_cast<const char*>(workspace);
    return launch_range_fill(reinterpret_cast<const unsigned*>(w + l.cnt), reinterpret_cast<const unsigned long long*>(w + l.cand), THR_CAP,
                             nq, lims, id_offset, D_out, I_out, st);
}

extern "C" int sss_ip_topk(const void* q, int64_t nq, const void* corpus, int64_t n, int d, int k, int dtype, int64_t id_offset,
                           float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                           size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return ip_topk_impl({.what = "ip_topk", .family = FAM_IP, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = dtype, .c_scan = corpus, .scan_dtype = dtype, .n = n,
                         .d = d, .k = k, .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status,
                         .unproven_count = unproven_count, .state = state, .state_bytes = state_bytes, .ws = workspace, .ws_bytes = workspace_bytes,
                         .st = static_cast<hipStream_t>(stream)});
}

extern "C" int sss_ip_topk_split(const float* q, int64_t nq, const float* corpus, const uint16_t* scan_image, int64_t n, int d, int k,
                                 int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                 int32_t* unproven_count, void* state, size_t state_bytes, void* workspace, size_t workspace_bytes,
                                 void* stream) {
    return ip_topk_impl({.what = "ip_topk_split", .family = FAM_IP, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = DT_F32, .c_scan = scan_image,
                         .scan_dtype = DT_SPLIT, .n = n, .d = d, .k = k, .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out,
                         .status = status, .unproven_count = unproven_count, .state = state, .state_bytes = state_bytes, .ws = workspace, .ws_bytes = workspace_bytes,
                         .st = static_cast<hipStream_t>(stream)});
}

extern "C" int sss_ip_topk_f16(const float* q, int64_t nq, const float* corpus, const uint16_t* scan_image, int corpus_shift,
                               float corpus_resid_norm, int64_t n, int d, int k, int64_t id_offset, float corpus_max_norm, float* D_out,
                               int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state, size_t state_bytes,
                               void* workspace, size_t workspace_bytes, void* stream) {
    return ip_topk_impl({.what = "ip_topk_f16", .family = FAM_IP, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = DT_F32, .c_scan = scan_image, .scan_dtype = DT_F16,
                         .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .n = n, .d = d, .k = k, .id_offset = id_offset,
                         .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status, .unproven_count = unproven_count, .state = state,
                         .state_bytes = state_bytes, .ws = workspace, .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

// ------------------------------------------------------------------------------------------
// L2 top-k on the same scans (include/sss_l2.h): float32 rows, the scan's keys biased by bias[row] = -|c_row|^2 / 2
// (rowops.hip: sss_l2_row_bias), scores the negated canonical squared distances (select_dev.h: err_bound_l2, DT_F32_L2).
extern "C" size_t sss_l2_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k, int scan_dtype) {
    return scans_f32_rows(scan_dtype) ? ip_topk_scan_workspace_bytes(nq, n, d, k, scan_dtype) : 0;
}

extern "C" int sss_l2_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                           float corpus_resid_norm, const float* bias, int64_t n, int d, int k, int64_t id_offset,
                           float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                           size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return ip_topk_impl({.what = "l2_topk", .family = FAM_L2, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = DT_F32, .c_scan = scan_image, .scan_dtype = scan_dtype,
                         .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .bias = bias, .n = n, .d = d, .k = k, .id_offset = id_offset,
                         .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status, .unproven_count = unproven_count, .state = state,
                         .state_bytes = state_bytes, .ws = workspace, .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

extern "C" size_t sss_l2_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d, int scan_dtype) {
    return scans_f32_rows(scan_dtype) ? sss_ip_topk_threshold_workspace_bytes(nsel, n, d, scan_dtype) : 0;
}

extern "C" int sss_l2_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                                     int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n, int d,
                                     int k, int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status,
                                     void* workspace, size_t workspace_bytes, void* stream) {
    return topk_threshold_impl({.what = "l2_topk_threshold", .family = FAM_L2, .q = q, .nq = nsel, .qsel = qsel, .c_exact = corpus, .exact_dtype = DT_F32,
                                .c_scan = scan_image, .scan_dtype = scan_dtype, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .bias = bias, .n = n,
                                .d = d, .k = k, .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status,
                                .ws = workspace, .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

// ------------------------------------------------------------------------------------------
// Scans at a width the row does not have (include/sss_pad.h): float32 rows of d_row elements, q and c_scan zero-extended to
// d_scan -- a width of scan_dtype's fused kernels -- by the builders of rowops.hip.  Zero columns add nothing to a dot
// product or to |c|^2, so the scan, its keys and its bound (for a chain of d_scan terms: what the scan really summed) are
// those of a d_scan-wide corpus; the select kernels re-score from the d_row-wide rows (SelectArgs::d_row).  A bias makes
// it the L2 search.
static bool pad_shape_ok(int d_row, int d_scan, int scan_dtype) {
    return d_row > 0 && d_row % 4 == 0 && d_row <= d_scan && scans_f32_rows(scan_dtype) && fused_shape_ok(d_scan, scan_dtype);
}

extern "C" size_t sss_pad_topk_workspace_bytes(int64_t nq, int64_t n, int d_row, int d_scan, int k, int scan_dtype) {
    return pad_shape_ok(d_row, d_scan, scan_dtype) ? ip_topk_scan_workspace_bytes(nq, n, d_scan, k, scan_dtype) : 0;
}

extern "C" int sss_pad_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                            float corpus_resid_norm, const float* bias, int64_t n, int d_row, int d_scan, int k, int64_t id_offset,
                            float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                            size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    return ip_topk_impl({.what = "pad_topk", .family = FAM_PAD, .q = q, .nq = nq, .c_exact = corpus, .exact_dtype = DT_F32, .c_scan = scan_image,
                         .scan_dtype = scan_dtype, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .bias = bias, .n = n, .d = d_scan, .d_row = d_row,
                         .k = k, .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out, .status = status,
                         .unproven_count = unproven_count, .state = state, .state_bytes = state_bytes, .ws = workspace, .ws_bytes = workspace_bytes,
                         .st = static_cast<hipStream_t>(stream)});
}

extern "C" size_t sss_pad_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d_row, int d_scan, int scan_dtype) {
    return pad_shape_ok(d_row, d_scan, scan_dtype) ? sss_ip_topk_threshold_workspace_bytes(nsel, n, d_scan, scan_dtype) : 0;
}

extern "C" int sss_pad_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                                      int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n,
                                      int d_row, int d_scan, int k, int64_t id_offset, float corpus_max_norm, float* D_out,
                                      int64_t* I_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream) {
    return topk_threshold_impl({.what = "pad_topk_threshold", .family = FAM_PAD, .q = q, .nq = nsel, .qsel = qsel, .c_exact = corpus, .exact_dtype = DT_F32,
                                .c_scan = scan_image, .scan_dtype = scan_dtype, .corpus_shift = corpus_shift, .corpus_resid = corpus_resid_norm, .bias = bias, .n = n,
                                .d = d_scan, .d_row = d_row, .k = k, .id_offset = id_offset, .corpus_max_norm = corpus_max_norm, .D_out = D_out, .I_out = I_out,
                                .status = status, .ws = workspace, .ws_bytes = workspace_bytes, .st = static_cast<hipStream_t>(stream)});
}

}  // namespace sss
