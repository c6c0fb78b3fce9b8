/* libsss, scoring a search result -- the primitive under the reference's retrieval metrics (test_amazon_filterd.py:
 * get_cur / future / all_jaccard :286-343, get_cur / all / future_recall :345-382, get_future_map :226-244, get_recall
 * :443-450; fine_tune_ours.py: get_score / get_ave_score :42-97): for every (query i, neighbour I[i, j]) pair the size of
 * the intersection of two item sets, then a small reduction per query.  Same library (libsss.so) and the same
 * conventions as include/sss.h and include/sss_sparse.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error (there is no workspace, so no -2);
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * An ITEM SET is the (ptr int64 [rows + 1], items int32) half of a session-vector CSR triple (sss_sparse.h): the
 * distinct item ids of a row in ASCENDING order, any length including 0; the weights are not read.
 */
#ifndef SSS_EVAL_H
#define SSS_EVAL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* inter[i, j] = |Q_i & C_r| and csize[i, j] = |C_r| with r = I[i, j] - id_offset, for the nq query sets (q_ptr, q_items)
 * against the n corpus sets (c_ptr, c_items); ptr entries index the triple's own items, so a sub-batch is
 * `ptr + first_row` with the same items.  I: int64 [nq, K]; inter, csize: int32 [nq, K], every entry written.
 * I[i, j] == -1 (the padding of a search with fewer than K results) is a MISSING neighbour: inter = 0, csize = -1.  Any
 * other id outside [id_offset, id_offset + n) is missing as well and ORs 1 into err (int32 [1], zeroed by the call).
 * Integer results: bit-reproducible.  0 < nq < 2^31, 0 < K <= 1024, 0 < n < 2^31; no pointer may be NULL (an empty
 * items array is still an allocation). */
int sss_item_overlap(const int64_t* q_ptr, const int32_t* q_items, int64_t nq, const int64_t* c_ptr, const int32_t* c_items,
                     int64_t n, const int64_t* I, int K, int64_t id_offset, int32_t* inter, int32_t* csize, int32_t* err,
                     void* stream);

/* Per-query sums over the K neighbours of sss_item_overlap's outputs; qsize int32 [nq] = |Q_i|; out double [nq, 4];
 * flags int32 [nq] (written, not OR-ed).  Every sum is accumulated in float64, SEQUENTIALLY IN ASCENDING j, so the
 * values are bit-reproducible.  With u = qsize + csize - inter (the union) per pair:
 *   out[i, 0] = sum_j (double)inter / (double)u            a pair with u == 0 adds 0 and sets flag bit 1
 *   out[i, 1] = sum_j (double)inter / (double)qsize        0 when qsize == 0, which sets flag bit 2
 *   out[i, 2] = the average precision of the hit vector (inter > 0) ranked by position: with h hits, hit t = 1..h at
 *               0-based position j_t, (sum_t (double)t / (double)(j_t + 1)) / (double)h; 0 when h == 0
 *   out[i, 3] = the number of j with (float)((double)inter / (double)u) > thr (a float32 comparison; u == 0 scores 0)
 * A missing neighbour (csize < 0) adds nothing to any of the four, is never a hit and sets no flag, but keeps its
 * rank: the positions j_t do not shrink.  0 < nq < 2^31, 0 < K <= 1024; no pointer may be NULL. */
int sss_overlap_metrics(const int32_t* inter, const int32_t* csize, const int32_t* qsize, int64_t nq, int K, float thr,
                        double* out, int32_t* flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
