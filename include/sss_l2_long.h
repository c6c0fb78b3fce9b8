/* libsss, L2 top-k of LONG float32 rows -- faiss IndexFlatL2.search at the reference's own vector width (D = 1600,
 * pretrain_filtered_amazon.py:281, under the 'l2' branch of its build_index, test_amazon_filterd.py:207-223), served by
 * the K-tiled matrix-core scan of sss_ip_topk_long (include/sss.h) instead of the exhaustive kernels.
 * Same library (libsss.so); the conventions are those of include/sss_l2.h:
 *
 *   - all buffers are CALLER-OWNED DEVICE pointers; nothing is allocated or freed here and there is no host
 *     synchronisation: work is enqueued on `stream` (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error; sss_last_error() (sss.h) returns the
 *     thread-local message of the last failure, which starts with the entry point's name without its sss_ prefix;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched, and a call that fails validation writes nothing.
 *
 * THE CONTRACT is that of sss_ip_topk_exhaustive at metric 1 (include/sss_l2.h spells it out): canonical float64
 * chain of squared differences rounded once to float32, results ordered by (distance asc, id asc), missing results
 * (+FLT_MAX, -1).  The scan only finds candidates: the key of (query, row) is sigma (q.c) + sigma bias[row], with
 * bias[row] = -|c_row|^2 / 2 (sss_l2_row_bias) and sigma the power of two the scaled float16 scan's scores live in,
 * moved down (sample levels) or up (last level) by the row's own error bound, which the scan derives from the bias;
 * every kept row is re-scored canonically from the float32 rows.
 *
 * Rows: float32, d % 64 == 0, d <= 4096 (the limits of sss_ip_topk_long for float32 rows); 0 < n < 2^31 - 1024;
 * k <= 1024.  scan_image / corpus_shift / corpus_resid_norm: the scaled float16 image of the rows, as for
 * sss_ip_topk_f16 (sss_scale_f16, sss_f16_resid_max), 16-byte aligned.  bias: n floats, 16-byte aligned.
 * corpus_max_norm: an upper bound of the largest row 2-norm; the caller takes this route only where
 * corpus_max_norm^2 / 2 is a finite, normal float32 (2^-60 <= corpus_max_norm <= 2^60 is what FlatIndex asks).
 */
#ifndef SSS_L2_LONG_H
#define SSS_L2_LONG_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* D_out [nq, k] float32 distances, I_out [nq, k] int64 = row + id_offset, status [nq] int32: 0 = exact; else the query
 * kept more rows than the candidate capacity (8192; 4096 for d > 2560) -- or its magnitudes put the scan's error bound
 * beyond float32 -- and must be re-run through sss_ip_topk_exhaustive at metric 1 (column k-1 of its row of D_out is an
 * upper bound of its true k-th distance, +FLT_MAX when none is known; the rest of the row is unspecified).
 * workspace: sss_l2_topk_long_workspace_bytes(nq, n, d) bytes, 256-byte aligned (0 for a shape this scan does not take). */
size_t sss_l2_topk_long_workspace_bytes(int64_t nq, int64_t n, int d);
int sss_l2_topk_long(const float* q, int64_t nq, const float* corpus, const void* scan_image, int corpus_shift,
                     float corpus_resid_norm, const float* bias, int64_t n, int d, int k, int64_t id_offset, float corpus_max_norm,
                     float* D_out, int64_t* I_out, int32_t* status, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
