// Internal interface between the scan kernel (scan.hip), the select / re-score kernels
// (select.hip, select_thr.hip) and the host orchestration of sss_ip_topk (ip_topk.hip).  gfx950 only.
#pragma once
#include "elem.h"

namespace sss {

// shift that maps a largest magnitude `amax` into [2^12, 2^13); 0 for an all-zero / non-finite row
__host__ __device__ inline int f16_shift(float amax) {
    if (!(amax > 0.f) || !(amax <= 3.4028234663852886e38f)) return 0;   // zero, NaN or inf
    int e;
    (void)frexpf(amax, &e);          // amax = m * 2^e, m in [0.5, 1)
    return 13 - e;
}

constexpr int KP = 16;          // per-lane candidate list length (register resident)
constexpr int WG_QUERIES = 256; // queries per scan workgroup (8 waves x 32)
constexpr int MAX_SLOTS = 128;  // admission-threshold slots per query (J <= MAX_SLOTS)
// A query's slot words start SLOT_STRIDE words apart whatever J is: the 1024 lines of a 1024-query batch then spread
// over 512 KB of address space -- and with it over the memory channels -- instead of sitting in 64 contiguous KB that
// every workgroup of the launch polls, fetches and hits with agent-scope atomics at the same moment (the bootstrap).
constexpr int SLOT_STRIDE = MAX_SLOTS;
constexpr unsigned ORD_NEG_INF = 0x007FFFFFu;   // f2ord(-inf); slot value 0 = "never written"
// One float32 ulp, as every proof of exactness allows for the final rounding of a score to float32 (select_dev.h: the
// proof window; exhaustive.hip: the bounded pre-test): relative to the score, with headroom over 2^-23 = 1.19e-7 ...
constexpr double ULP32_REL = 2.4e-7;
constexpr double ULP32_MIN = 1e-44;             // ... and its floor in the subnormal range (the spacing there is 2^-149 = 1.4e-45)

static inline int pow2_at_least(int x) { int p = 64; while (p < x) p <<= 1; return p; }   // smallest power of two >= max(x, 64): LDS key arrays

// Row shapes of sss_ip_topk_long: d % 64 == 0 and exact rows of at most 16384 bytes (k_select_all keeps the query row in
// LDS), scanned by what scan_pair_ok (elem.h) pairs them with.
static inline bool long_shape_ok(int d, int exact_dtype, int scan_dtype) {
    return d > 0 && d % 64 == 0 && d * elem_bytes(exact_dtype) <= 16384 && scan_pair_ok(exact_dtype, scan_dtype, true);
}

// One step of the canonical L2 chain (oracle/search_ref.canonical_l2; exhaustive.hip at metric 1 and the L2 re-score of
// select_dev.h): acc + (q - c)^2 in float64, one rounding per subtraction, multiplication and addition -- never fused.
__device__ __forceinline__ double l2_chain_step(double acc, double q, double c) {
    const double dl = __dsub_rn(q, c);
    return __dadd_rn(acc, __dmul_rn(dl, dl));
}

// STATE words (caller-owned, zero before the first call; every call leaves them zero: the select
// kernel, their last reader, clears what the call used -- no per-call memset launch).  Because the
// whole buffer is zero between calls, each call may lay it out as it likes:
//   slots   u32 [nq][SLOT_STRIDE]   admission-threshold slots: the first J words of a query's 512 bytes (J = 16: one 64-byte line)
//   cnt     u32 [nq]      candidates written per query        (at word nq * MAX_SLOTS)
//   maxlast u64 [nq]      largest tail key over FULL lists    (8-byte aligned, after cnt)
static inline size_t state_off_cnt(long nq) { return (size_t)nq * MAX_SLOTS; }                       // in words
static inline size_t state_off_maxlast(long nq) { return (state_off_cnt(nq) + (size_t)nq + 1) & ~(size_t)1; }
static inline size_t state_words(long nq) { return state_off_maxlast(nq) + 2 * (size_t)nq; }

// Per-search plan (host).  Workspace: cand u64 [nq][cap] compacted candidate keys, cap = L * KP.
struct ScanPlan {
    int G, S, L, K2, J, Ju, cert, boot, append, tile_rows;      // J slots per query = Ju classes; boot: the first tile of a split is scanned twice (max-only first)
    int tau_skip;                                               // cert == 1: the threshold is the (tau_skip + 1)-th smallest slot (16 - K2)
    int total_tiles, tiles_per_split, cap;
    size_t total_bytes;
};

ScanPlan make_plan(long nq, long n, int d, int k, int dtype);

struct ScanArgs {
    const void* Q;
    const void* C;
    int nq, n, tiles_per_split, total_tiles, S, G, J, Ju, cert, boot, append, cap;
    int tau_skip = 0;
    unsigned* slots;                // the three arrays live in the caller's state buffer
    unsigned* cnt;
    unsigned long long* maxlast;
    unsigned long long* cand;
    // threshold form only (k_scan<..., THR = true>): the compact query list and its per-query thresholds
    const int* qsel = nullptr;
    const float* thr = nullptr;
    // L2 scans only (k_scan<..., MET = 1>; appended, so the inner-product kernels read what they always read): the per-row
    // bias -|c|^2 / 2 every score starts from, and the DT_F16 image's corpus shift (a lane scales the bias by
    // 2^(corpus_shift + its query's shift))
    const float* bias = nullptr;
    int corpus_shift = 0;
};

ScanPlan make_thr_plan(long nsel, long n, int d, int scan_dtype, int cap);
int launch_scan(int dtype, int d, int tile_rows, const ScanArgs& a, hipStream_t st);
int launch_scan_l2(int dtype, int d, int tile_rows, const ScanArgs& a, hipStream_t st);     // (scan_l2.hip; launch_scan calls it when a.bias is set)

struct SelectArgs {
    const void* Q;
    const void* C;
    int nq, d, dtype, k, K2, J, cap;
    int tau_skip = 0;               // the scan's rank-selected threshold: (tau_skip + 1)-th smallest of the 16 slots
    int scan_dtype;                 // what produced the candidates (DT_F32 / DT_BF16 / DT_SPLIT / DT_F16 / DT_H16 / DT_I8): picks the error bound
    int corpus_shift;               // DT_F16: the corpus image is corpus * 2^corpus_shift (else 0)
    float corpus_resid;             // DT_F16: largest row norm of (image * 2^-corpus_shift - corpus)
    const unsigned long long* cand;
    unsigned* slots;                // state arrays: read, then cleared
    unsigned* cnt;
    unsigned long long* maxlast;
    long id_offset;
    float corpus_max_norm;
    float* D_out;
    long* I_out;
    int* status;
    int* unproven_count;        // optional device counter: += 1 per query left unproven
    int metric = 0;             // 1: L2 -- scan keys are q.c - |c|^2 / 2, scores are NEGATED squared distances (select_dev.h: query_bound)
    int d_row = 0;              // elements of a STORED row of C when it is narrower than the scan (include/sss_pad.h); 0: d.  Q stays [nq, d]
};

int launch_select(const SelectArgs& a, hipStream_t st);

// Threshold rung (select_thr.hip: k_thr_prepare, k_select_all; scan.hip: k_scan<..., THR = true>)
struct ThrArgs {
    const void* Q;                  // all queries [*, d] of the exact element type
    const void* C;                  // the stored rows (re-score)
    const int* qsel;                // [nsel] query rows to resolve
    int nsel, d, dtype, k, cap;
    long n;
    int scan_dtype, corpus_shift;
    float corpus_resid, corpus_max_norm;
    long id_offset;
    float* thr;                     // [nsel]   workspace
    unsigned* cnt;                  // [nsel]   workspace
    const unsigned long long* cand; // [nsel][cap] workspace
    float* D_out;                   // [nq, k]: row q's k-th entry is read (lower bound), rows of resolved queries are rewritten
    long* I_out;
    int* status;                    // [nq]: set to 0 for resolved queries
    double* qb = nullptr;           // optional [nsel][2] cache of the queries' (error bound, unscale): written by the first kernel
    int qb_ready = 0;               //   that computes them (qb_ready == 0), read by the later ones (sss_ip_topk_long: five kernels a search);
                                    //   metric 1: 2 [nsel] more doubles behind the pairs: the queries' off = -|q|^2, then
                                    //   the bound k_select_all prunes with (select_thr.hip: THE PER-ROW BOUND)
    int keep = 0;                   // k_thr_prepare: 1 = keep the rows already kept that pass the NEW threshold (compacted in place)
                                    //                instead of starting from an empty array (sss_ip_topk_long: disjoint levels)
    int metric = 0;                 // 1: L2 (as SelectArgs::metric; D_out holds distances: its column k-1 is an UPPER bound, negated on the way in)
    int d_row = 0;                  // as SelectArgs::d_row (k_select_all's re-score; the range kernels never see it set)
};
int launch_thr_prepare(const ThrArgs& a, hipStream_t st);
int launch_select_all(const ThrArgs& a, hipStream_t st);
// sss_ip_topk_long's fused steps: everything a search needs before its first scan in ONE launch (f16 query image when
// `qimg` is given, identity selection, D_out rows at -FLT_MAX, thresholds -inf, counters 0, status 1, the per-query
// (error bound, unscale) cache), and the step between two levels in one launch (bound from the level just scanned ->
// column k-1 of D_out -> the next level's threshold; counters zeroed, or -- a.keep -- the kept rows pruned in place).
// (seed: L2 only -- [2][2][nsel] floats, the seed coefficients of k_scan_long<DT_F16, 1> for lowered and for raised keys;
//  nullptr otherwise)
int launch_long_setup(const ThrArgs& a, int* qsel, void* qimg, float* seed, hipStream_t st);
int launch_bound_prepare(const ThrArgs& a, hipStream_t st);
// Range search, fused route (select_thr.hip): scan thresholds from per-query radii (identity selection written to `qsel`,
// counters zeroed); the canonical re-score + keep (> radius) + sort by id of the kept rows (counts / status per query,
// the entries left in the candidate rows); the copy of those entries to D / I at lims.
int launch_range_prepare(const ThrArgs& a, const float* radius, int* qsel, hipStream_t st);
int launch_range_select(const ThrArgs& a, const float* radius, long* counts, int* status, hipStream_t st);
int launch_range_fill(const unsigned* cnt, const unsigned long long* cand, int cap, long nq, const long* lims, long id_offset, float* D,
                      long* I, hipStream_t st);

// What a scanning search entry point was called with (host only: never a kernel argument).  Each extern "C" entry point
// of ip_topk.hip and scan_long.hip fills one, every field by name, and the checks, the workspace layouts and the kernel
// argument structs above are made from it.
enum Family { FAM_IP, FAM_L2, FAM_PAD };       // whose header's rules apply: include/sss.h, sss_l2.h + sss_l2_long.h, sss_pad.h
struct SearchCall {
    const char* what = nullptr; Family family = FAM_IP;             // the entry point's name in messages
    const void* q = nullptr; long nq = 0; const int* qsel = nullptr;   // queries of the exact element type, d wide; threshold forms: nq is nsel, the length of qsel
    const void* c_exact = nullptr; int exact_dtype = DT_F32;        // the stored rows the candidates are re-scored from ...
    const void* c_scan = nullptr; int scan_dtype = DT_F32;          // ... and what k_scan reads: the rows themselves or a scan-only image,
    int corpus_shift = 0; float corpus_resid = 0.f;                 //     a DT_F16 image with its shift and residual
    const float* bias = nullptr;                // set: an L2 search (keys q.c + bias[row], scores negated distances)
    long n = 0; int d = 0, d_row = 0, k = 0;    // d: the width of q and c_scan; d_row: of a stored row where it is narrower (sss_pad.h), else 0
    long id_offset = 0; float corpus_max_norm = 0.f;
    float* D_out = nullptr; long* I_out = nullptr; int* status = nullptr; int* unproven_count = nullptr;
    void* state = nullptr; size_t state_bytes = 0; void* ws = nullptr; size_t ws_bytes = 0;
    hipStream_t st = nullptr;
};

// What every scanning search entry point checks about its scan source (ip_topk.hip), in this order: the (exact, scan)
// element-type pairing and row shape (long_rows: long_shape_ok, else the fused scans' shapes), the image pointer and
// its 16-byte alignment, a DT_F16 image's corpus_shift in [-160, 160] and corpus_resid >= 0, n and nq below 2^31.
// SSS_EINVAL with a message that starts with c.what on the first failure.
int check_scan_source(const SearchCall& c, bool long_rows);
// The buffers the L2 and pad families require (ip_topk.hip), in this order: the row bias 16-byte aligned (bias_required:
// and there), q / corpus / D_out / I_out / status there, and -- aligned_rows, the pad family -- q and corpus 16-byte aligned.
int check_buffers(const SearchCall& c, bool bias_required, bool aligned_rows);
// The ThrArgs of a threshold-form search but for thr / cnt / cand, which the caller sets from its workspace layout.
ThrArgs thr_args(const SearchCall& c, int cap);

// a float32 [nsel][n] score matrix at the head of a workspace, up to the next 256-byte boundary
static inline size_t score_matrix_bytes(long nsel, long n) { return al256((size_t)nsel * n * 4); }
// scores [nsel][n] of the selected queries against every row (exhaustive.hip: k_exact_scores_rows where the shape has it, else
// k_exact_scores); lb / lb_by_row: the optional pre-test bound of k_exact_scores_rows (inner product only).
int launch_exact_scores(const void* q, const int* qsel, long nsel, const void* c, long n, int d, int dtype, int metric, float* scores,
                        const float* lb, int lb_by_row, hipStream_t st);
// the exact top-k of a finished [nsel][n] score matrix (topk_scores.hip): the tail of the exhaustive search, also sparse.hip's
constexpr int RS_MAX_K = 1024;
size_t topk_of_scores_bytes(long nsel, long n);
int topk_of_scores(const float* scores, const int* qsel, long nsel, long n, int k, long id_offset, int metric, float* D_out,
                   long* I_out, void* tail, hipStream_t st);

}  // namespace sss
