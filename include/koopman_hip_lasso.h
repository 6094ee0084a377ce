/* What the L1-constrained fit (kp_fit_lasso, kp_fit_lasso_batch, kp_fit with a lasso vector; kp_lasso.hip) ran, and its product
 * kernels alone (kp_symm_gemm.h).  Kept apart from koopman_hip.h, whose entry points the MATLAB gateway matlab/kp_mex.c covers
 * one for one: kp_symm_product serves tests and probes from C and Python and gets no gateway command. */
#ifndef KOOPMAN_HIP_LASSO_H
#define KOOPMAN_HIP_LASSO_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kp_timer_get(27): the kernels the iteration loop of the most recent lasso batch launched, as a bit mask (koopman_hip.h) */
#define KP_LASSO_RAN_EPT4 0x1u       /* kp_lasso_project_kernel<4>: up to 4 elements of V per thread, in registers */
#define KP_LASSO_RAN_EPT8 0x2u       /* <8> */
#define KP_LASSO_RAN_EPT16 0x4u      /* <16> */
#define KP_LASSO_RAN_EPT24 0x8u      /* <24> */
#define KP_LASSO_RAN_EPT0 0x10u      /* <0>: the slice of V goes through memory */
#define KP_LASSO_RAN_MULTI 0x20u     /* kp_lasso_v_kernel / kp_lasso_newton_kernel / kp_lasso_final_kernel: the multi-launch form */
#define KP_LASSO_RAN_SMALL 0x40u     /* kp_symm_gemm_kernel */
#define KP_LASSO_RAN_TILED 0x80u     /* kp_symm_gemm2_kernel<RA, RB> */
#define KP_LASSO_RAN_NAIVE 0x100u    /* kp_symm_gemm_naive_kernel */
#define KP_LASSO_RAN_RA4 0x200u      /* tiled with RA = 4; RA = 5 ... 8: 0x400, 0x800, 0x1000, 0x2000 (KP_LASSO_RAN_RA4 << (RA - 4)) */
#define KP_LASSO_RAN_RB2 0x4000u     /* tiled with RB = 2 */
#define KP_LASSO_RAN_RB3 0x8000u     /* 3 */
#define KP_LASSO_RAN_RB4 0x10000u    /* 4 */
#define KP_LASSO_RAN_RB6 0x20000u    /* 6 */

/* `variant` of kp_symm_product */
#define KP_SYMM_BY_SHAPE 0           /* what the solver runs at this shape */
#define KP_SYMM_SMALL 1              /* kp_symm_gemm_kernel (kp_symm_gemm_naive_kernel where W does not fit its LDS: W > 404) */
#define KP_SYMM_TILED_RB 10          /* + RB, RB = 2 ... 6: kp_symm_gemm2_kernel<RA, RB>, 16 RB columns per workgroup (also 2, 3: RB = 2, 4) */
/* `ran` of kp_symm_product */
#define KP_SYMM_RAN_SMALL 1
#define KP_SYMM_RAN_NAIVE 2
#define KP_SYMM_RAN_TILED 1000       /* + 10 RA + RB */

/* kp_symm_product: C (W x nc) = G (W x W, symmetric; only G = G' is meaningful) X (W x nc), host arrays, column-major f64 - one
 *   launch of the product kernels of the lasso iteration on the context's stream, nothing else.  `variant` is handed to the
 *   dispatch as it is: KP_SYMM_BY_SHAPE picks as the solver does (the small kernel for W < 48 or nc ceil(W / 16) <= 19000, else
 *   the tiled one with RA = 4 ... 8 by W and RB in {2, 3, 4, 6} by a cost model of the device's CU count), the other values
 *   force a kernel (an operand of 4 GB or more always takes the small kernel: the tiled one addresses with 32-bit offsets).
 *   The device result buffer holds a NaN in every element before the launch, so an element that no lane stores comes back
 *   as NaN.  ran (may be NULL): KP_SYMM_RAN_SMALL, KP_SYMM_RAN_NAIVE or KP_SYMM_RAN_TILED + 10 RA + RB.
 *   KP_ERR_ARG: W < 1, nc < 1, a NULL array, a variant other than 0, 1, 2, 3, 12 ... 16. */
int kp_symm_product(kp_ctx* ctx, const double* G, const double* X, int W, int nc, int variant, double* C, int* ran);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_LASSO_H */
