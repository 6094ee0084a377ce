/* Continuous-time models (kp_logm.hip, kp_ct_rollout.hip).  Kept apart from koopman_hip.h, whose entry points the MATLAB
 * gateway matlab/kp_mex.c covers one for one: these serve Ksysid's time_type = 'continuous' for C and Python callers. */
#ifndef KOOPMAN_HIP_CT_H
#define KOOPMAN_HIP_CT_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- matrix logarithm (the logm of get_model :1186-1187, get_BLmodel :1245-1246, get_NLmodel :1307-1310) ----
 * kp_logm: L_b = scale * logm(A_b + shift I) for nb column-major n x n matrices, one call.
 *   Inverse scaling and squaring without a Schur form: square roots by determinant-scaled product-form Denman-Beavers
 *   iterations (Gauss-Jordan inverses with partial pivoting, the determinant from their pivots) until
 *   ||A^(1/2^s) - I||_1 <= 0.25, then the 7-node Gauss-Legendre quadrature of log(I + X) = int_0^1 X (I + t X)^-1 dt
 *   (the [7/7] Pade approximant), L = scale 2^s log(I + X).
 *   status (nb): KP_OK, or KP_ERR_NOT_CONVERGED with L_b all NaN when no real principal logarithm is reached: a
 *   non-finite input, a negative determinant (an odd number of negative eigenvalues), an exactly singular pivot, a square
 *   root whose iteration did not converge within 50 steps (e.g. a pair of negative eigenvalues) or does not square back to
 *   its argument within 1e-8 relative (the Gauss-Jordan inverses of a nearly singular iterate, as of a rank-deficient K),
 *   more than 64 square roots.
 *   nsqrt (nb): square roots taken (may be NULL).  Each matrix's result is independent of the others in the batch.
 *   Limits: 1 <= n <= 512; KP_ERR_ARG beyond. */
int kp_logm(kp_ctx* ctx, int nb, int n, const double* A, double shift, double scale, double* L, int* nsqrt, int* status);

/* ---- continuous-time validation rollouts (val_model :1679-1683, val_BLmodel :1777-1781) ----
 * kp_rollout_ct: per sample interval z' = A z + B u (KP_MODEL_LINEAR) or z' = A z + sum_i u_i B_i z (KP_MODEL_BILINEAR)
 *   integrated over [0, Ts] with the input of the sample held, from the end point of the previous interval: ode45's
 *   Dormand-Prince 5(4) pair and step control (initial step, MaxStep Ts / 10, error norm max |e_i| / max(|y_i|, |ynew_i|,
 *   atol / rtol)).  Layouts as kp_rollout: A batch x [N x N], B batch x [N x mb] (mb = m or N m), z0 batch x N,
 *   U batch x [T x m], Y out batch x [T x n_out] (row t = the first n_out entries of the state at sample t).
 *   naccept / nreject (batch, may be NULL): accepted / rejected steps over the whole rollout.  status (batch): KP_OK, or
 *   KP_ERR_NOT_CONVERGED (step-size underflow, more than 100000 steps in one interval, a non-finite state) with the
 *   samples from the failing one on NaN.  Limits: 1 <= N <= 512, n_out <= N, rtol > 0, atol > 0, Ts > 0. */
int kp_rollout_ct(kp_ctx* ctx, int model_type, int batch, const double* A, const double* B, int N, int m, const double* z0,
                  const double* U, int T, int n_out, double Ts, double rtol, double atol, double* Y, int* naccept,
                  int* nreject, int* status);

/* kp_rollout_nl_ct: zeta' = Kf econ_full([zeta; u]) (val_NLmodel :1849-1856), the dictionary lifted in-kernel at every
 * stage; layouts as kp_rollout_nl (Kf batch x [nzeta x N], zeta0 batch x nzeta, U batch x [T x m], Z batch x [T x nzeta]),
 * step control, counts and status as kp_rollout_ct.  KP_ERR_ARG for a dictionary that is not of the nonlinear model
 * type or too large for the kernel's LDS (the limits of kp_rollout_nl). */
int kp_rollout_nl_ct(kp_ctx* ctx, const kp_basis* basis, int batch, const double* Kf, const double* zeta0, const double* U,
                     int T, double Ts, double rtol, double atol, double* Z, int* naccept, int* nreject, int* status);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_CT_H */
