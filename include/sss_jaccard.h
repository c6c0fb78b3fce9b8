/* libsss, ground truth -- a similarity the session encoder can be trained to approximate, over the WHOLE corpus: the
 * item-set kinds of the reference's get_score (fine_tune_ours.py:42-55, 'all_jaccard' and 'cur_jaccard'; the kind
 * CFG.sim_type is set to, 'all_product_type_score', is include/sss_ptype.h's), its exact top-k,
 * and the band counts / first rows that the fine-tuning triple mining (fine_tune_ours.py:187-235) and a thresholded recall
 * need.  Same library (libsss.so) and the same conventions as include/sss.h and include/sss_sparse.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).  The ONE exception is `edges` of sss_jaccard_bands: a
 *     HOST array, read before the launch and not afterwards;
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * THE CONTRACT (stated here once; everything else refers to it).
 *   An ITEM SET is the (ptr int64 [rows + 1], items int32) half of a session-vector CSR triple (sss_sparse.h): the distinct
 *   item ids of a row in ASCENDING order, any length including 0; weights are not read (as in sss_eval.h).  ptr entries
 *   index the triple's own items, so a sub-batch is `ptr + first_row` with the same items.
 *   For a query set Q and a corpus set C:  inter = |Q & C|,  uni = |Q| + |C| - inter.
 *   The SCORE OF RECORD is float32( (double)inter / (double)uni ), and 0 when uni == 0 (get_score('cur_jaccard')'s rule;
 *   for 'all_jaccard' the reference divides by zero there).
 *   For sets of at most 64 items (all that sss_session_vectors_* builds) the float32 order IS the order of the rationals:
 *   two distinct fractions with denominators <= 128 differ by at least 1 / 128^2 = 2^-14 relative to 1 >= either of them,
 *   far more than float32's 2^-24 rounding.  For larger caller-built sets the float32 score is the contract.
 *   Every result is an integer or one correctly rounded division: bit-reproducible, independent of the launch geometry.
 *   There are no floating-point atomics; integer atomics (add, min) carry the band totals across workgroups.
 */
#ifndef SSS_JACCARD_H
#define SSS_JACCARD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Exact top-k of nq query sets against n corpus sets by the score of record.  Writes D_out [nq, k] float32 and I_out
 * [nq, k] int64 = row + id_offset, the k best rows by (score desc, id asc); rows scoring 0 are ordinary results; missing
 * results (n < k): I = -1, D = -FLT_MAX.  0 < nq <= 65535, 0 < n < 2^31, 0 < k <= 1024 (the limits of sss_sparse_topk); no
 * pointer may be NULL (an empty items array is still an allocation); workspace: sss_jaccard_topk_workspace_bytes(nq, n)
 * bytes, 256-byte aligned (the [nq, n] score matrix and the selection's buffers; nothing is carried between calls). */
size_t sss_jaccard_topk_workspace_bytes(int64_t nq, int64_t n);
int sss_jaccard_topk(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                     int64_t n, int k, int64_t id_offset, float* D_out, int64_t* I_out, void* workspace, size_t workspace_bytes,
                     void* stream);

/* Bands.  edges: HOST array of n_edges float64 values, 1 <= n_edges <= 7, finite and strictly ascending.  The band of a
 * (query, row) pair is the number of j with (double)inter / (double)uni >= edges[j] -- a FLOAT64 comparison, the
 * arithmetic of the reference's Python; a pair with uni == 0 has the ratio 0.  Writes counts [nq, n_edges + 1] int64, the
 * rows of every band, and first [nq, n_edges + 1] int64, the lowest row + id_offset of the band, -1 when it has none.
 * Both are initialised here, on the stream; no score matrix is written and there is no workspace.  With edges (0.2, 0.8)
 * bands 2 / 1 / 0 are the reference's pos / half_pos / neg picks; `score > t` is the edge nextafter(t, +inf).
 * 0 < nq <= 65535, 0 < n < 2^31, 0 <= id_offset <= 2^63 - 1 - n (so that -1 is no row's id); no pointer may be NULL. */
int sss_jaccard_bands(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                      int64_t n, const double* edges, int n_edges, int64_t id_offset, int64_t* counts, int64_t* first,
                      void* stream);

#ifdef __cplusplus
}
#endif
#endif
