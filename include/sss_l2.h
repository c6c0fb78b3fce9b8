/* libsss, L2 top-k on the matrix-core scans -- faiss IndexFlatL2.search, the 'l2' branch of the reference's build_index
 * (test_amazon_filterd.py:207-223), served by the candidate scans of include/sss.h instead of the exhaustive kernels.
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
 * THE CONTRACT is that of sss_ip_topk_exhaustive at metric 1: the distance of (query, row) is sum_k (q_k - c_k)^2
 * accumulated sequentially in float64 over the stored float32 elements (one rounding per subtraction, multiplication
 * and addition) and rounded once to float32; results are ordered by (distance asc, id asc); missing results are
 * (+FLT_MAX, -1).  The scan only finds candidates: since |q - c|^2 = |q|^2 - 2 (q.c - |c|^2 / 2), the nearest rows are
 * those with the largest key q.c + bias[row], bias[row] = -|c_row|^2 / 2, and a key is what the inner-product scan
 * computes with every accumulator started from its row's bias.  Candidates are re-scored canonically from the float32
 * rows and every query is proven exact or flagged in `status`, as for sss_ip_topk.
 *
 * Rows: float32, d in {64, 128, 256} for scan_dtype 0 (the rows themselves) and 2 (the bf16 hi|lo image,
 * sss_split_bf16), d in {128, 256, 512} for scan_dtype 3 (the scaled float16 image, sss_scale_f16, with its
 * corpus_shift and corpus_resid_norm as for sss_ip_topk_f16; both ignored otherwise).  0 < n < 2^31 - 1024.
 * corpus_max_norm: an upper bound of the largest row 2-norm (sss_row_norm_max); the caller takes this route only
 * where corpus_max_norm^2 / 2 is a finite, normal float32 (2^-60 <= corpus_max_norm <= 2^60 is what FlatIndex asks).
 */
#ifndef SSS_L2_H
#define SSS_L2_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* bias[i] = -|c_i|^2 / 2 for the n float32 rows of `corpus` (d % 4 == 0): the sum of squares in float64, rounded once
 * to float32.  One array per corpus, shared by all three scans.  n == 0 is a no-op.  The searches below take a bias
 * array of n floats, 16-byte aligned; entries behind row n - 1 are never read. */
int sss_l2_row_bias(const float* corpus, int64_t n, int d, float* bias, void* stream);

/* L2 top-k of nq float32 queries.  scan_image: what scan_dtype names (scan_dtype 0: the rows themselves, = corpus),
 * 16-byte aligned.  D_out [nq, k] float32 distances, I_out [nq, k] int64 = row + id_offset, status [nq] int32:
 * 0 = proven exact, else re-run the query through sss_l2_topk_threshold and, if still set, sss_ip_topk_exhaustive at
 * metric 1 (column k-1 of an unproven query's row of D_out is an upper bound of its true k-th distance, +FLT_MAX when
 * none is known).  unproven_count: optional int32 [1], += 1 per unproven query.  k <= 500.  state: the buffer
 * sss_ip_topk_state_bytes(nq) sizes, zero before the first call and left zero by every call (16-byte aligned);
 * workspace: sss_l2_topk_workspace_bytes(nq, n, d, k, scan_dtype) bytes, 256-byte aligned (0 for a shape without a scan). */
size_t sss_l2_topk_workspace_bytes(int64_t nq, int64_t n, int d, int k, int scan_dtype);
int sss_l2_topk(const float* q, int64_t nq, const float* corpus, const void* scan_image, int scan_dtype, int corpus_shift,
                float corpus_resid_norm, const float* bias, int64_t n, int d, int k, int64_t id_offset, float corpus_max_norm,
                float* D_out, int64_t* I_out, int32_t* status, int32_t* unproven_count, void* state, size_t state_bytes,
                void* workspace, size_t workspace_bytes, void* stream);

/* Threshold rung for the nsel query rows qsel (int32, rows of q) that sss_l2_topk left unproven: one more scan keeps
 * every row whose distance could still reach the k-th distance already known (column k-1 of the query's row of D_out)
 * and re-scores all of them.  Rows of D_out / I_out of resolved queries are rewritten and their status set to 0; a
 * query with more than 8192 such rows keeps its status.  k <= 8192.  workspace:
 * sss_l2_topk_threshold_workspace_bytes(nsel, n, d, scan_dtype) bytes, 256-byte aligned. */
size_t sss_l2_topk_threshold_workspace_bytes(int64_t nsel, int64_t n, int d, int scan_dtype);
int sss_l2_topk_threshold(const float* q, const int32_t* qsel, int64_t nsel, const float* corpus, const void* scan_image,
                          int scan_dtype, int corpus_shift, float corpus_resid_norm, const float* bias, int64_t n, int d, int k,
                          int64_t id_offset, float corpus_max_norm, float* D_out, int64_t* I_out, int32_t* status, void* workspace,
                          size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
