/* libsss, the query text encoder -- the three row kernels of NodeTextTransformer (the reference's query-node encoder,
 * model/NodeEmbedding.py:62-98: nn.Embedding * sqrt(ninp) + sinusoidal positions, post-norm nn.TransformerEncoder layers,
 * mean over the token axis) on PACKED token rows: the rows of every sequence are contiguous, ptr int32 [n_seq + 1] gives
 * each sequence's row range.  The four GEMMs of a layer are sss_linear_grouped and the pooling is sss_segment_reduce
 * (sss.h).  Same library (libsss.so) and the same conventions as include/sss.h:
 *
 * Conventions (every entry point):
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error (a failed launch); there is no workspace, so -2 is never
 *     returned; sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * Every output row is written over its whole leading dimension: the columns past the row's width are written as zeros,
 * so a row can be the K = pad32(width) operand of the next GEMM as it stands.  DESIGN.md section 5.9 has the computation.
 */
#ifndef SSS_TEXT_H
#define SSS_TEXT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x[r, :e] = table[tok[r], :] * scale + pe[pos[r], :] for r < n, as a rounded product followed by a rounded sum (no fused
 * multiply-add: the float32 result of `embedding(src) * sqrt(ninp) + pe` bit for bit); x[r, e:ld_x] = 0.
 * table [n_token, e] and pe [n_pos, e] are dense (row stride e).  A row whose token id is outside [0, n_token) or whose
 * position is outside [0, n_pos) is written as zeros and sets *err (int32, device, zeroed by the caller) to 1; nothing is
 * read out of bounds.  Limits: e % 4 == 0, 4 <= e <= 1024, ld_x % 4 == 0 and >= e, n_token, n_pos >= 1, 0 <= n < 2^31,
 * table / pe / x 16-byte aligned and non-null, tok / pos / err non-null.  n == 0 returns 0 without a launch once the
 * scalar arguments are checked (an empty batch has no buffers to check).  Messages start with "text_embed:". */
int sss_text_embed(const float* table, int64_t n_token, const float* pe, int64_t n_pos, const int64_t* tok, const int32_t* pos,
                   int64_t n, int e, float scale, float* x, int64_t ld_x, int32_t* err, void* stream);

typedef struct {
    const float* qkv; int64_t ld_qkv;       /* [n_rows, >= 3 e], e = heads * head_dim: the q | k | v column blocks of   */
                                            /* one GEMM output; head eta owns columns [eta D, (eta + 1) D) of each block */
    const int32_t* ptr;                     /* [n_seq + 1] row range of each sequence                                   */
    const uint8_t* key_ok;                  /* [n_rows] 1: the row is a key; 0: it attends but is not attended to       */
    int64_t n_rows;
    int64_t n_seq;
    int32_t heads;
    int32_t head_dim;                       /* 1 .. 64, any value (the reference's is 50)                               */
    int32_t max_len;                        /* 1 .. 64: no sequence has more rows (the caller checks; the kernel clamps) */
    float* out; int64_t ld_out;             /* [n_rows, >= e]; must not alias qkv                                       */
} sss_seq_attention_args;

/* Multi-head self-attention inside each packed sequence:
 *     out[r, eta, :] = sum_j softmax_j(< q[r, eta, :], k[j, eta, :] >) v[j, eta, :]
 * over the rows j of r's own sequence with key_ok[j]; the maximum is subtracted before exp.  1 / sqrt(D) is NOT applied:
 * the caller folds it into the q rows of in_proj.  A sequence with no valid key writes zeros; out[r, e:ld_out] = 0.
 * Row ranges are clamped to [0, n_rows] and to max_len rows, so a bad ptr cannot cause an access out of bounds (rows left
 * out by the clamp are not written).  No atomics; the result does not depend on the launch geometry and is
 * bit-reproducible.
 * Limits: 1 <= head_dim <= 64, heads >= 1, e = heads * head_dim <= 1024 (any e: no vector access is made, so neither e nor
 * a leading dimension need be a multiple of 4 here; the encoder's e is, for the kernels around this one), 1 <= max_len <= 64,
 * ld_qkv >= 3 e, ld_out >= e, 0 <= n_seq, n_rows < 2^31, every pointer non-null, qkv and out 4-byte aligned.
 * n_seq == 0 or n_rows == 0 returns 0 without a launch once the scalar arguments are checked.  Messages start with
 * "seq_attention:". */
int sss_seq_attention(const sss_seq_attention_args* args, void* stream);

/* y[r, :e] = LayerNorm(x[r, :e] + res[r, :e]) * gamma + beta for r < n; y[r, e:ld_y] = 0.  Two passes inside the row: the
 * mean, then the sum of squared deviations from it (biased variance) plus eps -- never E[x^2] - E[x]^2.  y may be exactly x
 * (in place, same leading dimension) and may not otherwise overlap an input.
 * Limits: e % 4 == 0, 4 <= e <= 1024, every leading dimension % 4 == 0 and >= e, eps > 0, 0 <= n < 2^31, every pointer
 * 16-byte aligned and non-null.  n == 0 returns 0 without a launch once the scalar arguments are checked.  Messages start
 * with "add_layernorm:". */
int sss_add_layernorm(const float* x, int64_t ld_x, const float* res, int64_t ld_res, const float* gamma, const float* beta,
                      float eps, int64_t n, int e, float* y, int64_t ld_y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
