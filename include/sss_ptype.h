/* libsss, ground truth under the product-type kind -- the similarity the reference is CONFIGURED with: config.py:61 sets
 * CFG.sim_type = 'all_product_type_score', the kind of get_score (fine_tune_ours.py:66-85) that its triple mining
 * (:187-235), the ground truth test() records (:887, :902) and the first figure main2 prints after a search
 * (test_amazon_filterd.py:670) all use: the cosine of two sessions' product-type count vectors.  This header is to that kind
 * what include/sss_jaccard.h is to the item-set kinds: the bags, their exact top-k, the band counts / first rows of the
 * mining, and the pair scores of a result.  Same library (libsss.so) and the same conventions as include/sss.h,
 * include/sss_sparse.h and include/sss_jaccard.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream).  The ONE exception is `edges` of sss_ptype_bands: a
 *     HOST array, read before the launch and not afterwards;
 *   - return 0 on success, -1 bad argument, -2 workspace too small, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * THE CONTRACT (stated here once; everything else refers to it).
 *   A TYPE BAG is a session-vector CSR triple (sss_sparse.h): `items` holds the DISTINCT product-type ids of a session in
 *   ASCENDING order (int32), `weights` the count of each type as a float32 -- a positive integer, exact -- and an empty row
 *   is a session without a typed item.  ptr entries index the triple's own items / weights, so a sub-batch is
 *   `ptr + first_row` with the same items and weights.
 *   For a query bag Q and a corpus bag C:  dot = sum_t q_t c_t,  nq2 = sum_t q_t^2,  nc2 = sum_t c_t^2 -- three integers.
 *   The SCORE OF RECORD is the float64
 *       dot == 0 ? 0.0 : __ddiv_rn((double)dot, __dsqrt_rn((double)(nq2 * nc2)))
 *   -- integer arithmetic, one correctly rounded square root and one correctly rounded division.  A bag without a typed item
 *   scores 0 against everything (the reference's zero vector).  Bags sss_type_bags_* builds have at most 64 actions, so
 *   nq2, nc2 <= 4096.  Caller-built bags are valid while every row's sum of squared counts is <= 2^26: then dot < 2^31 and
 *   nq2 * nc2 <= 2^52, exact in a double (the Python layer checks this once per batch; the kernels do not).
 *   Top-k scores are float32(score), the order (float32 score desc, id asc), sss_sparse_topk's rule.  Bands compare the
 *   float64 score with >=, as sss_jaccard_bands does.  Pair scores are the float64 value itself.
 *   Every result is bit-reproducible and independent of the launch geometry.  There are no floating-point atomics; integer
 *   atomics (add, min) carry the band totals across workgroups.
 *
 * DEVIATION from the reference: it divides each count vector by its float64 norm first and sums the products in
 *   first-occurrence order of the types, so its float64 value depends on that order, can exceed 1 and can fall on either side
 *   of a threshold it should sit on (measured: at most 4 ulp from the score of record).  The score of record
 *   puts a pair of exactly parallel bags at 1.0 and a pair with dot^2 * 25 == 16 * nq2 * nc2 at the double nearest 0.8.
 */
#ifndef SSS_PTYPE_H
#define SSS_PTYPE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Type bags of every session of an action table in its device form (sess_ptr int64 [n_sessions + 1], is_search uint8 and
 * item_id int64 per action, as sss_session_vectors_*), through item_type int32 [n_items]: the product type of every item,
 * -1 for an item without one (the reference's `action[4] is None`).  Every non-search action whose item has a type adds
 * one to its type's count: counts are over ACTIONS, not distinct items.  The two-step protocol of sss_session_vectors_*:
 * _count writes counts int32 [n_sessions], the distinct types of every session (and zeroes `err`); the caller takes their
 * exclusive prefix sum as ptr int64 [n_sessions + 1]; _fill writes items int32 / weights float32 [ptr[n_sessions]].
 * err int32 [1], OR-ed: 1 = a session with more than 64 item actions (typed or not) or a decreasing sess_ptr, 2 = an item
 * id outside [0, n_items), 4 = a type id outside [-1, n_types).  A flagged session is an empty row, in both steps alike.
 * 0 < n_sessions < 2^31, 0 < n_items < 2^31, 0 < n_types < 2^31; no pointer may be NULL. */
int sss_type_bags_count(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                        const int32_t* item_type, int64_t n_items, int64_t n_types, int32_t* counts, int32_t* err, void* stream);
int sss_type_bags_fill(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                       const int32_t* item_type, int64_t n_items, int64_t n_types, const int64_t* ptr, int32_t* items,
                       float* weights, int32_t* err, void* stream);

/* Exact top-k of nq query bags against n corpus bags by the score of record.  Writes D_out [nq, k] float32 and I_out
 * [nq, k] int64 = row + id_offset, the k best rows by (float32 score desc, id asc); rows scoring 0 are ordinary results;
 * missing results (n < k): I = -1, D = -FLT_MAX.  0 < nq <= 65535, 0 < n < 2^31, 0 < k <= 1024 (the limits of
 * sss_jaccard_topk); no pointer may be NULL (an empty items array is still an allocation); workspace:
 * sss_ptype_topk_workspace_bytes(nq, n) bytes, 256-byte aligned (the [nq, n] score matrix and the selection's buffers;
 * nothing is carried between calls). */
size_t sss_ptype_topk_workspace_bytes(int64_t nq, int64_t n);
int sss_ptype_topk(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                   const int32_t* c_items, const float* c_weights, int64_t n, int k, int64_t id_offset, float* D_out,
                   int64_t* I_out, void* workspace, size_t workspace_bytes, void* stream);

/* Bands: sss_jaccard_bands with the weights.  edges: HOST array of n_edges float64 values, 1 <= n_edges <= 7, finite and
 * strictly ascending.  The band of a (query, row) pair is the number of j with score >= edges[j], the float64 score of
 * record.  Writes counts [nq, n_edges + 1] int64, the rows of every band, and first [nq, n_edges + 1] int64, the lowest
 * row + id_offset of the band, -1 when it has none.  Both are initialised here, on the stream; no score matrix is written
 * and there is no workspace.  With edges (0.2, 0.8) bands 2 / 1 / 0 are the reference's pos / half_pos / neg picks;
 * `score > t` is the edge nextafter(t, +inf).  0 < nq <= 65535, 0 < n < 2^31, 0 <= id_offset <= 2^63 - 1 - n; no pointer
 * may be NULL. */
int sss_ptype_bands(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                    const int32_t* c_items, const float* c_weights, int64_t n, const double* edges, int n_edges, int64_t id_offset,
                    int64_t* counts, int64_t* first, void* stream);

/* Pair scores of a result: for I int64 [nq, K] writes scores double [nq, K], the score of record of (query i, row
 * I[i, j] - id_offset).  I[i, j] == -1 is a missing neighbour and scores NaN; any other id outside
 * [id_offset, id_offset + n) is missing too and ORs 1 into err int32 [1] (zeroed here, on the stream) -- sss_item_overlap's
 * rules.  0 < nq < 2^31, 0 < K <= 1024, 0 < n < 2^31; no pointer may be NULL. */
int sss_ptype_pair_scores(const int64_t* q_ptr, const int32_t* q_items, const float* q_weights, int64_t nq, const int64_t* c_ptr,
                          const int32_t* c_items, const float* c_weights, int64_t n, const int64_t* I, int K, int64_t id_offset,
                          double* scores, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
