/* libsss, the reduced-precision grouped GEMM -- sss_linear_grouped (sss.h) with both operands of the product rounded to
 * bfloat16 and the sum kept in float32, on the bf16 matrix cores.  Opt-in: text.BertNodeEncoder(gemm="bf16") and
 * text.NodeTextTransformer(gemm="bf16") run their dense layers on it.  Same library (libsss.so)
 * and the same conventions as sss_linear_grouped; this header lives in include/lowp/ and is bound through
 * _lib.LOWP_HEADERS.
 *
 * Conventions:
 *   - all buffers are CALLER-OWNED DEVICE pointers (tensor.data_ptr()); nothing is allocated
 *     or freed here and there is no host synchronisation: work is enqueued on `stream`
 *     (a hipStream_t passed as void*; NULL = the default stream);
 *   - return 0 on success, -1 bad argument, -3 HIP error (there is no workspace, so no -2);
 *     sss_last_error() (sss.h) returns the thread-local message of the last failure;
 *   - re-entrant per stream; no global state except the error string;
 *   - arguments are validated before anything is launched.
 *
 * THE ERROR CONTRACT, per output element before the activation.  Let x^ = bf16(x), the float32 input rounded to nearest
 * even (NaN and +-inf pass through), w^ the stored bf16 weight, and s = sum_k x^_k w^_k the exact real sum; every product
 * of two bf16 values is exact in float32.  The value v that goes into the activation satisfies
 *     |v - (s + bias)|  <=  K * 2^-23 * sum_k |x^_k w^_k|  +  2^-23 * |s + bias|
 * one float32 ulp per accumulation step (2^-23, not 2^-24: the rounding of the matrix pipe's internal adders is not
 * documented, and one ulp covers truncation as well) and one for the bias add.  bfloat16 SUBNORMAL inputs (|x^| or |w^|
 * below 2^-126) are NOT covered: how the matrix pipe treats them is unverified.  Bias, the activations 0..5 and the post
 * stage are the float32 arithmetic of sss_linear_grouped, instruction for instruction; the output is float32.
 * The order of the sum depends on K alone, never on n, m, the row, the column or the other problems of the launch: a row's
 * result does not change with its neighbours, and a problem's result does not change with the launch it is part of.
 */
#ifndef SSS_LINEAR_BF16_H
#define SSS_LINEAR_BF16_H
#include <stddef.h>
#include <stdint.h>
#include "../sss.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Up to 4 problems  y[n, m] = act(bf16(x)[n, k] w[m, k]^T + bias)  (+ the post stage) in ONE launch, the struct of sss.h
 * unchanged except for how two fields are read:
 *   w     points at uint16_t bf16 BITS, row-major [m, >= k] (convert float32 weights once with sss_f32_to_bf16);
 *   ldw   counts bf16 elements: ldw % 8 == 0, ldw >= k.
 * x stays float32 (ldx % 4 == 0, ldx >= k) and is rounded on its way into the kernel; y, bias, post_scale, post_shift are
 * float32 (ldy >= m).  k % 32 == 0, shared by all problems; n >= 0, m > 0; act 0..5; post_scale and post_shift come
 * together.  There is no gather mode: ids, table and xcopy must be NULL. */
int sss_linear_grouped_bf16(const sss_linear_problem* problems, int n_problems, int k, void* stream);

#ifdef __cplusplus
}
#endif
#endif
