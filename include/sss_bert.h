/* libsss, the node text encoder -- the embedding stage of a BERT encoder (the reference's PretrainedQAEAEncoder,
 * model/NodeEmbedding.py:100-125: a BertModel without its pooling layer, a masked mean over the tokens and an optional
 * Linear) on PACKED token rows, as in include/sss_text.h.  Everything after the embedding stage is an entry point that
 * exists: the GEMMs of a layer are the grouped linear of sss.h (its act = 5 is the exact GELU of the feed-forward block),
 * the attention and the add + LayerNorm are those of sss_text.h, the pooling and the scatter of de-duplicated rows are the
 * segment reduction and the row gather of sss.h.  Same library (libsss.so) and the same conventions as include/sss.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error (a failed launch); there is no workspace, so -2 is never
 *     returned; the last-error string of sss.h holds the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * Every output row is written over its whole leading dimension: the columns past the row's width are written as zeros,
 * so a row can be the K = pad32(width) operand of the next GEMM as it stands.  DESIGN.md section 5.10 has the computation.
 */
#ifndef SSS_BERT_H
#define SSS_BERT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x[r, :e] = LayerNorm((word[tok[r]] + type[tt[r]]) + pos[p[r]]) * gamma + beta for r < n; x[r, e:ld_x] = 0.
 * The two float32 sums are taken in exactly that order (BertEmbeddings.forward: inputs_embeds + token_type_embeddings,
 * then + position_embeddings); there is no multiplication before the LayerNorm, so nothing can be fused across them.
 * The LayerNorm is two passes inside the row: the mean, then the sum of squared deviations from it (biased variance) plus
 * eps -- never E[x^2] - E[x]^2 -- so a row of one repeated value comes out as beta exactly, whatever eps (BERT's is 1e-12).
 * word [n_word, e], type [n_type, e] and pos [n_pos, e] are dense (row stride e); gamma, beta [e].
 * A row whose tok is outside [0, n_word), whose tt is outside [0, n_type) or whose p is outside [0, n_pos) is written as
 * zeros and sets *err (int32, device, zeroed by the caller) to 1; nothing is read out of bounds.
 * Limits: e % 4 == 0, 4 <= e <= 1024, ld_x % 4 == 0 and >= e, n_word, n_type, n_pos >= 1, eps > 0, 0 <= n < 2^31,
 * word / type / pos / gamma / beta / x 16-byte aligned and non-null, tok / tt / p / err non-null.  n == 0 returns 0 without
 * a launch once the scalar arguments are checked (an empty batch has no buffers to check).  Messages start with
 * "bert_embed:". */
int sss_bert_embed(const float* word, int64_t n_word, const float* type, int64_t n_type, const float* pos, int64_t n_pos,
                   const int64_t* tok, const int32_t* tt, const int32_t* p, const float* gamma, const float* beta, float eps,
                   int64_t n, int e, float* x, int64_t ld_x, int32_t* err, void* stream);

#ifdef __cplusplus
}
#endif
#endif
