/* libsss, the session-graph builder with the two outputs of the reference's sequence_to_graph
 * (util_amazon_filtered.py:98-230) that sss_graph_counts / sss_graph_fill of include/sss.h do not produce:
 * ignore_query=True (:101-103; CFG.ignore_query, config.py:8 -- every graph the reference's pre-training builds) and
 * data['product'].last_click_mask (:203-216, read by SRGNN_Pooling, model/gnn.py:173).
 * Same library (libsss.so) and the same conventions as include/sss.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error;
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure, which starts with the entry
 *     point's name without its sss_ prefix;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched, and a call that fails validation writes nothing.
 *
 * The action table, bases, scratch, err and sss_graph_out are those of sss_graph_counts / sss_graph_fill (sss.h); the
 * two steps and the read-back of the five totals between them are the same.  With flags == 0 and both new pointers NULL
 * the _ex calls ARE the old calls for every valid argument list: the same kernels, the same bytes.  (They are stricter on
 * invalid ones: NULL sess_ptr / bases / scratch / err / out and n_sessions <= 0 return -1 here before anything is launched.)
 *
 * flags: bit 0 = SSS_GRAPH_IGNORE_QUERY; any other bit set is a bad argument (-1, nothing written).  Both steps of one
 * build take the same flags.
 *
 * SSS_GRAPH_IGNORE_QUERY: the graphs of the click-only sessions, as if every search action had been dropped from the
 * table first.  The session length is its click count nclk, a click's position id is nclk - (its rank among the
 * clicks), the root is the only query node of its graph (q_x 0, q_pos nclk; bases row 0 counts exactly one per session,
 * Nq == n_sessions) and every click edge starts at it.  Product nodes, first-occurrence order, transitions and weights
 * are unchanged: they never depended on the searches.  A session without clicks is root + the "unknown item" node.
 * query_tok is not read (it may be NULL); is_search is.  The limit stays 64 RAW actions per session (*err != 0
 * otherwise), however few of them are clicks: a wave's lanes are the raw actions in both modes.
 *
 * last_click_mask: float32 [Np] or NULL.  1.0 at the product node of the session's last click (the "unknown item" node of
 * a session without clicks), 0.0 at every other node: the reference's mask, its products numbered in first-occurrence
 * order.  Every element is written.
 * last_node: int32 [n_sessions] or NULL.  The batch-global id of that node, one per graph (last_click_mask[last_node[g]]
 * == 1.0), for callers that gather instead of summing under the mask. */
#ifndef SSS_GRAPH_H
#define SSS_GRAPH_H
#include <stddef.h>
#include <stdint.h>

#include "sss.h"
#ifdef __cplusplus
extern "C" {
#endif

#define SSS_GRAPH_IGNORE_QUERY 1

int sss_graph_counts_ex(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id, int64_t n_sessions,
                        int flags, int32_t* bases, int32_t* scratch, int32_t* err, void* stream);
int sss_graph_fill_ex(const int64_t* sess_ptr, const uint8_t* is_search, const int64_t* item_id,
                      const int64_t* query_tok, int64_t n_sessions, int flags, const int32_t* bases,
                      const sss_graph_out* out, float* last_click_mask, int32_t* last_node, void* stream);

#ifdef __cplusplus
}
#endif
#endif
