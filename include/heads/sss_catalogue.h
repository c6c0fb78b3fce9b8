/* libsss, the catalogue heads -- the trained model's own item prediction over the whole catalogue, at inference time: the
 * binary cross-entropy the reference validates on (get_next_product_asin_loss, train_subsession_embedding.py:271-302;
 * get_all_product_asin_loss, train_session_embedding.py:122-) without the [B, V] matrices it materialises, and the hit count
 * of get_next / get_all_product_asin_accuracy.  Same library (libsss.so) and the same conventions as sss.h; this header lives
 * in include/heads/ and is bound through _lib.HEADS_HEADERS.  Python: sessionsimilaritysearch_amd/catalogue.py; DESIGN.md
 * section 5.13.
 *
 * Conventions:
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * THE CONTRACT of sss_catalogue_bce.  rep [b, kp] are the sessions' representations (the head's output), table [v, ldw]
 * the item embedding, both zero-extended to kp columns; row r's target items are items[ptr[r] .. ptr[r+1]), strictly
 * ascending and inside [0, v): the CSR layout of sparse.SessionVectors.
 *
 *   LOGIT.  s[r][i] is the float32 fma chain of sss_linear_grouped (sss.h) with no bias, in its k order: starting from
 *     +0, one correctly rounded fmaf per k; per 32-wide chunk k0, for u = 0..3, for i = 0..3: k0+8u+i, then k0+8u+4+i
 *     (oracle_linear_chain).  The kernel keeps k_linear_grouped's per-chunk v_mfma_f32_32x32x2_f32 order, so the logit is
 *     the same bits as sss_linear's output element.
 *   TERMS.  softplus(z) = max(z, 0) + log1pf(expf(-|z|)), in float32.  A positive pair (i in row r's target set)
 *     contributes  clamp(softplus(-s), SSS_CATALOGUE_P_LO, SSS_CATALOGUE_P_HI)  to sums[r][0]; a kept negative contributes
 *     clamp(softplus(s), SSS_CATALOGUE_N_LO, SSS_CATALOGUE_N_HI)  to sums[r][1].  The four limits are the reference's
 *     val = clip(sigmoid(s), 1e-4, 0.9999) moved into the log domain: -log of fl32(0.9999) and of fl32(1e-4) for
 *     -log(val), -log of 1 - fl32(1e-4) and of 1 - fl32(0.9999) (float32 subtractions) for -log(1 - val), each evaluated in
 *     float64 and rounded to float32.  THE ONE NUMERICAL DEVIATION from the reference: this is its mathematics without the
 *     cancellation of its own float32 log(1 - val); the reference's loss differs from this one by that rounding.
 *   KEPT NEGATIVES.  mode = 1: every non-target item.  mode = 0: a non-target item i of global row g = row_offset + r is
 *     kept iff  H(seed, g, i) < keep_thr, with H the upper 32 bits of the SplitMix64 finaliser of a 64-bit counter:
 *         x = seed + (g * v + i) * 0x9E3779B97F4A7C15          (all arithmetic modulo 2^64)
 *         x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9
 *         x = (x ^ (x >> 27)) * 0x94D049BB133111EB
 *         x =  x ^ (x >> 31);          H = x >> 32
 *     The caller computes keep_thr = floor(min(1, n_neg / v) * 2^32) (the reference's rate 1000 / v is n_neg = 1000) and
 *     calls mode = 1 where that reaches 2^32.  The mask is a function of (seed, g, i) only.
 *   COUNTS.  counts[r][0] = the row's targets, counts[r][1] = its kept negatives: exact.
 *   SUMS.  sums[r][*] are float64 sums of the float32 terms.  No floating-point atomics: a workgroup adds the terms of
 *     SSS_CATALOGUE_SPAN consecutive items per (row, item lane) in ascending item order, combines the 64 lanes in a fixed
 *     tree and writes one partial per (span, row); a second kernel adds a row's partials in ascending span order.  A row's
 *     four outputs depend on that row of rep, its targets, the table, seed and g alone -- never on b, on the row's
 *     neighbours or on how the caller chunks the batch (with matching row_offset) -- and two runs give the same bits.
 *   NaN.  A NaN logit of a positive or kept pair makes that row's sum NaN; the kernel does not look for it.
 */
#ifndef SSS_CATALOGUE_H
#define SSS_CATALOGUE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* the clamp limits (hexadecimal float32 literals; decimal in the comment) */
#define SSS_CATALOGUE_P_LO 0x1.a3855ep-14f /* -log(fl32(0.9999))     = 1.0002159e-4 */
#define SSS_CATALOGUE_P_HI 0x1.26bb1cp+3f  /* -log(fl32(1e-4))       = 9.2103405    */
#define SSS_CATALOGUE_N_LO 0x1.a3855ep-14f /* -log(1 - fl32(1e-4))   = 1.0002159e-4 */
#define SSS_CATALOGUE_N_HI 0x1.26b9c0p+3f  /* -log(1 - fl32(0.9999)) = 9.2101746    */
/* items whose terms one workgroup adds up before it writes a partial (a multiple of the 64-item tile) */
#define SSS_CATALOGUE_SPAN 1024

/* Bytes of workspace sss_catalogue_bce needs for b rows against v items: the per-(span, row) partials. */
size_t sss_catalogue_bce_workspace_bytes(int64_t b, int64_t v);

/* The loss parts of b rows: sums [b, 2] float64 (positive part, negative part) and counts [b, 2] int64, as the contract
 * above states them.  rep [b, kp] float32, dense; table [v, ldw] float32; kp % 32 == 0, ldw >= kp, ldw % 4 == 0;
 * 0 < v < 2^31; 0 <= b <= 4194240; mode 0 or 1 (keep_thr and seed are ignored under mode 1); row_offset >= 0.  b == 0
 * returns 0 and touches nothing. */
int sss_catalogue_bce(const float* rep, const float* table, int64_t ldw, int kp, const int64_t* ptr, const int32_t* items,
                      int64_t b, int64_t v, int mode, uint32_t keep_thr, uint64_t seed, int64_t row_offset, double* sums,
                      int64_t* counts, void* workspace, size_t workspace_bytes, void* stream);

/* hits[r] = the number of DISTINCT entries of I[r][0 .. k) that lie in row r's set items[ptr[r] .. ptr[r+1]) (strictly
 * ascending), found by binary search; an entry outside [0, 2^31) -- the padding -1 -- is in no set.  I [b, k] int64,
 * 0 < k <= 1024, 0 <= b < 2^31; b == 0 returns 0. */
int sss_catalogue_hits(const int64_t* I, int64_t b, int k, const int64_t* ptr, const int32_t* items, int32_t* hits,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif
