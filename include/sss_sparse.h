/* libsss, sparse session index -- the SKNN / STAN item-vector baselines of the reference's retrieval entry point
 * (test_amazon_filterd.py: sequence_to_binary_vec :48-57, sequence_to_stan_vec :37-46, find_K_sparse_dense :403-412,
 * the 'SKNN' / 'STAN' branch of main2 :582-603).  Same library (libsss.so) and the same conventions as include/sss.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * A SESSION VECTOR is a sparse row over the items [0, n_items): the distinct item ids of the session's non-search
 * actions in ASCENDING order (int32) and one float32 weight per item.  A batch of them is a CSR triple
 * (ptr int64 [rows + 1], items int32 [ptr[rows]], weights float32 [ptr[rows]]).  Weights are computed in float64 and
 * rounded once to float32 (m distinct items, L item actions, i = 0..L-1 an action's position among them):
 *   mode 0, binary (SKNN, and every corpus row):  w = 1 / sqrt(m)
 *   mode 1, stan:  u[item] = sum over the item's occurrences, in action order, of exp((i - L) / lammy);
 *                  w = u / sqrt(sum of u^2 in ascending item order)
 * A session without item actions is an empty row; item id 0 is an ordinary item.
 */
#ifndef SSS_SPARSE_H
#define SSS_SPARSE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Session vectors from the device form of an action table (sess_ptr int64 [n_sessions + 1], is_search uint8 [T],
 * item_id int64 [T]; the inputs of sss_graph_counts), in two steps: sss_session_vectors_count writes the number of
 * distinct items of every session (counts int32 [n_sessions]); the caller turns them into ptr (exclusive prefix sum,
 * int64 [n_sessions + 1]) and allocates items / weights of ptr[n_sessions] entries; sss_session_vectors_fill writes
 * them.  err (int32 [1]): zeroed by the count, then OR-ed by both calls with 1 = a session with more than 64 item
 * actions (or a decreasing sess_ptr), 2 = an item id outside [0, n_items); a flagged session is an empty row.
 * lammy: the decay of mode 1, finite and > 0 (ignored by mode 0).  0 < n_sessions < 2^31, 0 < n_items < 2^31. */
int sss_session_vectors_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                              int64_t n_items, int32_t* counts, int32_t* err, void* stream);
int sss_session_vectors_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                             int64_t n_items, int mode, double lammy, const int64_t* ptr, int32_t* items, float* weights,
                             int32_t* err, void* stream);

/* Exact top-k of nq query vectors against n corpus vectors (both CSR triples as above; ptr entries index the triple's
 * own items / weights, so a sub-batch is `ptr + first_row` with the same items / weights).  The canonical score of
 * (query, row) is the float64 sum of (double)wq * (double)wc over the shared items in ascending item order, rounded
 * once to float32; a pair without a shared item scores 0 and is an ordinary result.  Writes D_out [nq, k] float32 and
 * I_out [nq, k] int64 = row + id_offset, the k best rows by (score desc, id asc); missing results (n < k): I = -1,
 * D = -FLT_MAX.  Bit-reproducible from run to run.  0 < nq <= 65535, 0 < n < 2^31, 0 < k <= 1024; no pointer may be
 * NULL (an empty items array is still an allocation); workspace: sss_sparse_topk_workspace_bytes(nq, n) bytes, 256-byte
 * aligned (the [nq, n] score matrix and the selection's buffers; nothing is carried between calls). */
size_t sss_sparse_topk_workspace_bytes(int64_t nq, int64_t n);
int sss_sparse_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                    const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                    int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
