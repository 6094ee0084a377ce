/* The Koopman spectrum (kp_eig_general.hip).  Kept apart from koopman_hip.h, whose entry points the MATLAB gateway
 * matlab/kp_mex.c covers one for one: this one serves Ksysid.spectrum for C and Python callers and gets no gateway command. */
#ifndef KOOPMAN_HIP_SPECTRUM_H
#define KOOPMAN_HIP_SPECTRUM_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KP_EIG_MAXN 512      /* the limit of kp_logm */
#define KP_EIG_WAVE_MAX 32   /* regime 1: one wave per matrix up to this order */
/* Regime 2 keeps the matrix in LDS.  With ld = n | 1 <= n + 1 the kernel asks for nmat n ld + 4 n + 64 doubles (nmat = 2,
 * H and Z, with vectors; 1, H alone, for values only; 4 n + 64: the reflector, wr, wi, the balancing scales and the reduction
 * slots), and 160 KB hold 20480:
 *   with vectors  2 n (n + 1) + 4 n + 64 <= 20480  <=>  n <= 99
 *   values only     n (n + 1) + 4 n + 64 <= 20480  <=>  n <= 140 */
#define KP_EIG_LDS_MAXN_VEC 99
#define KP_EIG_LDS_MAXN_VAL 140
#define KP_EIG_MAX_ITER 30   /* QR iterations per eigenvalue; exceptional shifts at 10 and 20 */

/* kp_eig: eigenvalues and, with want_vectors, right eigenvectors of nb column-major n x n real matrices (the layout of
 *   kp_logm), one matrix per workgroup, one launch.  The classical real algorithm: balancing by powers of two without
 *   permutation, Householder reduction to Hessenberg form, Francis double-shift QR with deflation (exceptional shifts at
 *   iterations 10 and 20 of an eigenvalue, at most KP_EIG_MAX_ITER), back-substitution on the quasi-triangular T, V = Z X,
 *   the balancing undone, every vector scaled to unit 2-norm.
 *   wr, wi (nb x n): slot i holds the eigenvalue that deflated at diagonal position i of T; a complex pair occupies
 *   consecutive slots, the one with positive imaginary part first.
 *   V (nb x [n x n] column-major; may be NULL when want_vectors == 0): the packed real form of LAPACK's dgeev - a real
 *   eigenvalue has one real column, a pair has columns j, j + 1 holding the real and imaginary part of the vector of the
 *   eigenvalue with positive imaginary part.
 *   iters (nb, may be NULL): QR iterations taken.  status (nb): KP_OK, or KP_ERR_NOT_CONVERGED with that matrix's outputs
 *   all NaN - a non-finite input, or an eigenvalue that did not deflate within KP_EIG_MAX_ITER iterations.  The call
 *   itself still returns KP_OK.  A matrix's result does not depend on nb or on its index in the batch, bit for bit.
 *   Regimes (kp_timer_get 23 reports which one the last call ran; 22 its kernel time, ms): 1 - n <= KP_EIG_WAVE_MAX, a
 *   64-thread workgroup, H and Z in LDS (the formula above: 18 432 bytes at n = 32 with vectors, 2 592 at n = 10); 2 - 256
 *   threads, LDS-resident up to KP_EIG_LDS_MAXN_VEC / _VAL; 3 - 256 threads, H and Z in a workspace slot (L2-resident).
 *   2 and 3 are one body and return the same bits.  Environment variable
 *   KP_EIG_REGIME (read per call; tests and A/B runs only) forces 2 or 3 where the shape admits it; 3 is always admitted.
 *   KP_ERR_ARG: nb < 1, n < 1, n > KP_EIG_MAXN, NULL A / wr / wi / status, want_vectors with NULL V. */
int kp_eig(kp_ctx* ctx, int nb, int n, const double* A, int want_vectors, double* wr, double* wi, double* V, int* iters,
           int* status);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_SPECTRUM_H */
