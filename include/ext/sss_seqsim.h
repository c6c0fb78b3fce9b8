/* libsss, the string metrics of a search result -- Levenshtein.seqratio over two lists of strings for every (query i,
 * neighbour I[i, j]) pair (fine_tune_ours.py: get_score 'all_query_score' / 'all_product_title_score' :56-65) and
 * get_string_match's two counts (util_amazon_filtered.py:239-249; test_amazon_filterd.py: get_query_metric :416-441).
 * Same library (libsss.so) and the same conventions as include/sss_eval.h; this header lives in include/ext/ and is bound
 * through _lib.EXT_HEADERS.
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
 * A STRING TABLE is (str_ptr int64 [n_strings + 1], str_chars int32): string u is the code points
 * str_chars[str_ptr[u] .. str_ptr[u + 1]), at most SSS_STR_MAX_CHARS of them, every one >= 0.  A SEQUENCE SET is
 * (ptr int64 [rows + 1], ids int32): row s is the string ids ids[ptr[s] .. ptr[s + 1]) in action order, repeats kept
 * (a sequence is not a set), at most SSS_SEQ_MAX_STRINGS of them.
 *
 * THE SCORE OF RECORD, float64, every operation rounded once, nothing fused:
 *   d(a, b)      the indel distance of two strings: len(a) + len(b) - 2 LCS(a, b); L = len(a) + len(b)
 *   match(a, b)  L == 0 or L > 10 d                       (Levenshtein.ratio(a, b) > 0.9, decided in integers)
 *   c(a, b)      (2.0 / (double)L) * (double)d, the division rounded first; 0.0 when L == 0
 *   T            [n1 + 1][n2 + 1]: T[i][0] = i, T[0][j] = j,
 *                T[i][j] = min(T[i-1][j] + 1.0, T[i][j-1] + 1.0, T[i-1][j-1] + c(A[i-1], B[j-1]))
 *   seqratio     ((double)(n1 + n2) - T[n1][n2]) / (double)(n1 + n2); 1.0 when n1 + n2 == 0
 */
#ifndef SSS_SEQSIM_H
#define SSS_SEQSIM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define SSS_SEQ_MAX_STRINGS 64      /* strings per sequence */
#define SSS_STR_MAX_CHARS 1024      /* code points per string */

/* For the nq query sequences (q_ptr, q_ids) against the n corpus sequences (c_ptr, c_ids), both over the one string table,
 * and every pair (i, j) with r = I[i, j] - id_offset  (I: int64 [nq, K]; all four outputs [nq, K], every entry written):
 *   ratio  double  seqratio(Q_i, C_r)
 *   qmatch int32   the strings of Q_i that match some string of C_r   (positions, so a repeated string counts twice)
 *   cmatch int32   the strings of C_r that match some string of Q_i
 *   clen   int32   len(C_r)
 * I[i, j] == -1 (the padding of a search with fewer than K results) is a MISSING neighbour: ratio = NaN, qmatch = cmatch =
 * 0, clen = -1.  Any other id outside [id_offset, id_offset + n) is missing as well and ORs 1 into err (int32 [1], zeroed
 * by the call).  Nothing is ever truncated: a pair with a sequence longer than SSS_SEQ_MAX_STRINGS, a string longer than
 * SSS_STR_MAX_CHARS or a string id outside [0, n_strings) is missing and ORs 2 into err.  Every value has one owner and
 * one order of operations: bit-reproducible.
 * 0 < n_strings < 2^31, 0 < nq < 2^31, nq * K < 2^31, 0 < K <= 1024, 0 < n < 2^31; no pointer may be NULL (an empty
 * chars or ids array is still an allocation). */
int sss_seq_pair_scores(const int64_t* str_ptr, const int32_t* str_chars, int64_t n_strings, const int64_t* q_ptr,
                        const int32_t* q_ids, int64_t nq, const int64_t* c_ptr, const int32_t* c_ids, int64_t n, const int64_t* I,
                        int K, int64_t id_offset, double* ratio, int32_t* qmatch, int32_t* cmatch, int32_t* clen, int32_t* err,
                        void* stream);

/* get_query_metric's two per-query sums over the K neighbours of sss_seq_pair_scores' outputs; qlen int32 [nq] =
 * len(Q_i); out double [nq, 2].  Float64, SEQUENTIALLY IN ASCENDING j: bit-reproducible.
 *   out[i, 0] = sum_j (double)(qmatch + cmatch) / (double)(qlen + clen)     a pair with qlen + clen == 0 adds 0
 *   out[i, 1] = sum_j (double)qmatch / (double)qlen                         0 when qlen == 0
 * A missing neighbour (clen < 0) adds nothing to either.  0 < nq < 2^31, 0 < K <= 1024; no pointer may be NULL. */
int sss_seq_query_metric(const int32_t* qmatch, const int32_t* cmatch, const int32_t* clen, const int32_t* qlen, int64_t nq,
                         int K, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
