/* libsss, matrix-core scans for float32 rows of ANY width d_row % 4 == 0 up to 512 -- the reference's default embedding
 * width 200 (config.py: emb_len) among them -- where include/sss.h and include/sss_l2.h serve d = 64 / 128 / 256 / 512 only.
 * Same library (libsss.so) and the same conventions as include/sss.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure, which starts with the entry
 *     point's name without its sss_ prefix;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched, and a call that fails validation writes nothing.
 *
 * THE ROUTE.  The scan image of the corpus and the query batch are built d_scan wide, d_scan the next width the chosen
 * scan has, with columns d_row .. d_scan-1 exact +0 (the builders below).  Zero columns add nothing to a dot product or
 * to |c|^2: the scan's keys, thresholds and error bound are those of a d_scan-wide corpus (the bound is taken for a
 * chain of d_scan terms -- what the scan really summed).  Candidates are re-scored from the STORED rows, d_row wide: the
 * canonical float64 chain of sss_ip_topk_exhaustive over exactly the row's elements, in order.  THE CONTRACT is therefore
 * that of sss_ip_topk (bias == NULL: scores, (score desc, id asc), missing (-FLT_MAX, -1)) or of sss_l2_topk (bias given:
 * squared distances, (distance asc, id asc), missing (+FLT_MAX, -1)) on the d_row-wide rows.
 *
 * scan_dtype and d_scan: 0 (float32 rows padded by sss_pad_rows_f32) and 2 (the bf16 hi|lo image, sss_pad_split_bf16):
 * d_scan in {64, 128, 256}; 3 (the scaled float16 image, sss_pad_scale_f16, with corpus_shift from sss_f16_shift of the
 * rows' largest magnitude and corpus_resid_norm from sss_pad_f16_resid_max; both ignored otherwise): d_scan in
 * {128, 256, 512}.  d_row % 4 == 0, 0 < d_row <= d_scan (d_row == d_scan is the unpadded search).  0 < n < 2^31 - 1024.
 */
#ifndef SSS_PAD_H
#define SSS_PAD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Row-widening builders: n float32 rows of d elements -> n rows of ds elements, columns d .. ds-1 exact +0.
 * d % 4 == 0, ds % 8 == 0, 0 < d <= ds; x and y 16-byte aligned; n == 0 is a no-op.
 *   sss_pad_rows_f32       y float32 [n, ds]: the rows themselves.  Pads the query batch of every search below and
 *                          builds the scan_dtype 0 image.
 *   sss_pad_scale_f16      y float16 [n, ds] = x * 2^shift rounded to nearest even (sss_scale_f16's rule; shift from
 *                          sss_f16_shift of the largest |element|, |shift| <= 160).
 *   sss_pad_split_bf16     y bfloat16 [n, 2 ds] = [hi(ds) | lo(ds)], hi = rne(x), lo = rne(x - hi) (sss_split_bf16's rule).
 *   sss_pad_f16_resid_max  *out (float32, zeroed by the caller) = max(*out, max over rows of |y_i * 2^-shift - x_i|_2),
 *                          x [n, d] against its image y [n, ds] of sss_pad_scale_f16: the corpus_resid_norm of the searches. */
int sss_pad_rows_f32(const float* x, int64_t n, int d, int ds, float* y, void* stream);
int sss_pad_scale_f16(const float* x, int64_t n, int d, int ds, int shift, uint16_t* y, void* stream);
int sss_pad_split_bf16(const float* x, int64_t n, int d, int ds, uint16_t* y, void* stream);
int sss_pad_f16_resid_max(const float* x, const uint16_t* y, int64_t n, int d, int ds, int shift, float* out, void* stream);

/* Top-k of nq queries.  q: float32 [nq, d_scan], the queries padded by sss_pad_rows_f32; corpus: float32 [n, d_row], the
 * stored rows; scan_image: what scan_dtype names, d_scan wide; all 16-byte aligned.  bias: NULL for inner product, else
 * the L2 row bias of the STORED rows (sss_l2_row_bias(corpus, n, d_row, ...): n floats, 16-byte aligned) and the search is
 * sss_l2_topk's.  D_out / I_out / status / unproven_count / state / workspace as for sss_ip_topk; k <= 500.  An unproven
 * query goes through sss_pad_topk_threshold and, if still set, sss_ip_topk_exhaustive with the UNPADDED queries at d_row.
 * workspace: sss_pad_topk_workspace_bytes(nq, n, d_row, d_scan, k, scan_dtype) bytes, 256-byte aligned (0 for an
 * unsupported shape); state: sss_ip_topk_state_bytes(nq) bytes, zero before the first call, left zero by every call. */
size_t sss_pad_topk_workspace_bytes(int64_t nq, int64_t n, int d_row, int d_scan, int k, int scan_dtype);
int sss_pad_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                 float corpus_resid_norm, const float* bias, int64_t n, int d_row, int d_scan, int k, int64_t id_offset,
                 float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state,
                 size_t state_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* Threshold rung for the nsel query rows qsel (int32, rows of q) that sss_pad_topk left unproven, as
 * sss_ip_topk_threshold (bias == NULL) / sss_l2_topk_threshold: resolved rows of D_out / I_out are rewritten and their
 * status set to 0; a query with more than 8192 rows above its threshold keeps its status.  k <= 8192.  workspace:
 * sss_pad_topk_threshold_workspace_bytes(nsel, n, d_row, d_scan, scan_dtype) bytes, 256-byte aligned. */
size_t sss_pad_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d_row, int d_scan, int scan_dtype);
int sss_pad_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                           int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n, int d_row,
                           int d_scan, int k, int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out,
                           int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
