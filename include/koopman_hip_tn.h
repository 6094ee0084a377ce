/* The TN product of the wide path alone (kp_tn_gemm.h: C = beta C + alpha A'B on the f64 matrix pipe; under the wide Gram matrices
 * of kp_wide.hip, the blocked factorisation and block substitution of kp_solve.hip and every step of kp_logm).  Kept apart from
 * koopman_hip.h, whose entry points the MATLAB gateway matlab/kp_mex.c covers one for one: kp_tn_product serves tests and probes
 * from C and Python and gets no gateway command. */
#ifndef KOOPMAN_HIP_TN_H
#define KOOPMAN_HIP_TN_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of kp_tn_product */
#define KP_TN_MISALIGN 0x1           /* A and B start 8 bytes past a 16-byte boundary: the 8-byte staging path, also with even lda, ldb */
#define KP_TN_SAME 0x2               /* B is the same device array as A (N == M, ldb == lda; the host B is ignored) */
#define KP_TN_MIRROR 0x4             /* kp_mirror_upper_kernel on C after the product (N == M) */

/* `ran` of kp_tn_product: KP_TN_RAN_FORM form + KP_TN_RAN_VEC vec + splits */
#define KP_TN_RAN_FORM 1000          /* x the form: 0 ... 3 the index of tng_shapes() (128 x 64, 128 x 96, 256 x 96, 192 x 128), 4 the 64 x 64 form */
#define KP_TN_RAN_VEC 100            /* x 1 when the 16-byte staging kernel was launched */
#define KP_TN_FORM_SMALL 4

/* kp_tn_product: C (M x N, ldc) = beta C + alpha (diag(wa wb) A)' B,  A: K x M (lda), B: K x N (ldb), host arrays, column-major
 *   f64 - one call of kp_tn_gemm on the context's stream, nothing else.  C is in/out: all ldc N doubles the host passes are
 *   uploaded before the launch and the whole buffer comes back, so the caller sees every element the device did and did not
 *   write.  Of A and B the (M - 1) lda + K and (N - 1) ldb + K doubles from their start are read; the rows K ... ld - 1 of
 *   the last column are NaN on the device.  wa, wb: length K, or NULL (weight 1).  tri: upper tiles only.  nsplit: contraction
 *   splits asked for (1 ... 64; the partial buffer holds all-ones bytes, a NaN in every element, before the launch, so a
 *   partial the reduction reads but no workgroup wrote shows).  form: -1 as the library picks, 0 ... 3 that index of
 *   tng_shapes(); M <= 64 always takes the 64 x 64 form.  ran (may be NULL): KP_TN_RAN_FORM form + KP_TN_RAN_VEC vec + the
 *   split count kp_tn_gemm ends up with.
 *   KP_ERR_ARG: a NULL A or C, a NULL B without KP_TN_SAME, M, N or K < 1, lda < K, ldb < K, ldc < M, form outside -1 ... 3,
 *   an unknown flag bit, KP_TN_SAME or KP_TN_MIRROR with N != M, KP_TN_SAME with ldb != lda, nsplit outside 1 ... 64.
 *   KP_ERR_HIP when kp_tn_gemm refuses the call (leading dimensions beyond its 32-bit tile offsets): C is left as it was. */
int kp_tn_product(kp_ctx* ctx, const double* A, int64_t lda, const double* B, int64_t ldb, int M, int N, int K,
                  double* C, int64_t ldc, double alpha, double beta, int tri, int nsplit,
                  const double* wa, const double* wb, int form, int flags, int* ran);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_TN_H */
