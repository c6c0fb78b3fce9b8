/* libsss, the HGT encoder -- the attention aggregation of PyG's HGTConv (the reference's third GNN, model/gnn.py:9-41:
 * HGT(800, 4 heads, 3 layers) of the two-tower session / sub-session model) on the project's CSR-by-target batches, and
 * the skip connection that closes a layer.  Same library (libsss.so) and the same conventions as include/sss.h:
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
 * THE COMPUTATION (DESIGN.md section 5.8 derives it from HGTConv).  For ONE target node type and one or two edge-type
 * SLOTS e, each a CSR by target (rowptr int32 [n_dst + 1], col int32 = source rows, the layout of every other kernel
 * here) with its own source rows k^e, v^e [n_src, heads * head_dim] (head eta owns columns [eta D, (eta + 1) D)):
 *     alpha_e(j -> i, eta) = < q[i, eta, :], k^e[j, eta, :] >                 -- a plain dot product: the caller has
 *                                                                                folded a_rel, p_rel / sqrt(D) into k^e
 *     w = exp(alpha - max) / (sum exp(alpha - max) + 1e-16)                  -- over the edges of i INSIDE slot e
 *     out[i, eta, :] = act( sum_e sum_j w * v^e[j, eta, :] )                 -- act = exact (erf) gelu when `gelu`
 *   A target with no incoming edge in a slot gets zeros from it.  One pass over the edges (online softmax): every k | v
 *   source row is read once.  No atomics; the result does not depend on the launch geometry and is bit-reproducible.
 */
#ifndef SSS_HGT_H
#define SSS_HGT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const float* k; int64_t ld_k;           /* [n_src, heads * head_dim], row stride ld_k                       */
    const float* v; int64_t ld_v;           /* likewise; k and v may be neighbouring column blocks of one buffer */
    const int32_t* rowptr;                  /* [n_dst + 1]                                                      */
    const int32_t* col;                     /* [rowptr[n_dst]] source rows; duplicates are ordinary edges       */
} sss_hgt_slot;

typedef struct {
    const float* q; int64_t ld_q;           /* [n_dst, heads * head_dim]                                        */
    sss_hgt_slot slot[2];
    int32_t n_slots;                        /* 1 or 2                                                           */
    int64_t n_dst;
    int32_t heads;                          /* 1, 2, 4 or 8                                                     */
    int32_t head_dim;                       /* % 4 == 0; heads * head_dim <= 2048                               */
    int32_t gelu;                           /* 0: none, otherwise x * 0.5 * (1 + erf(x / sqrt(2)))              */
    float* out; int64_t ld_out;             /* [n_dst, heads * head_dim]; must not alias an input               */
} sss_hgt_args;

/* Limits: heads in {1, 2, 4, 8}, head_dim % 4 == 0, heads * head_dim <= 2048, every leading dimension a multiple of 4
 * and at least heads * head_dim, every pointer 16-byte aligned and non-null, 0 <= n_dst < 2^31.  n_dst == 0 returns 0
 * without a launch once the scalar arguments are checked (an empty batch has no buffers to check).  Messages start with
 * "hgt_aggregate:". */
int sss_hgt_aggregate(const sss_hgt_args* args, void* stream);

/* y[r, :h] += beta * x[r, :h] for r < n: the (1 - sigmoid(skip)) * x half of HGTConv's skip connection (the sigmoid(skip)
 * factor of the other half is folded into a_lin's weights).  h % 4 == 0, leading dimensions multiples of 4 and >= h,
 * 0 <= n < 2^31; n == 0 returns 0 without a launch, as above.  Messages start with "hgt_skip:". */
int sss_hgt_skip(float* y, int64_t ld_y, const float* x, int64_t ld_x, float beta, int64_t n, int h, void* stream);

#ifdef __cplusplus
}
#endif
#endif
