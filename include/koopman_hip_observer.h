/* Batched load observer of a loaded Koopman model (kp_observer.hip).  Kept apart from koopman_hip.h, whose entry points
 * the MATLAB gateway matlab/kp_mex.c covers one for one: MATLAB keeps the reference's Ksysid.observer_load /
 * val_observer_load(_sparse), these are for C and Python callers. */
#ifndef KOOPMAN_HIP_OBSERVER_H
#define KOOPMAN_HIP_OBSERVER_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KP_OBS_RATE = 1, KP_OBS_PIN_LAST = 2 };   /* flags of kp_load_observe */

/* ---- load observer (replaces Ksysid.observer_load, Ksysid.m:1978-2030, called once per window by val_observer_load
 * :2033-2075 and val_observer_load_sparse :2079-2139) ----
 * kp_load_observe: the load estimate of nwin windows of hor rows, one call.
 *   basis: the UNLOADED dictionary (linear or bilinear; N = basis N, psi = econ_full), model_type KP_MODEL_LINEAR or
 *   KP_MODEL_BILINEAR, A: NL x NL and B: NL x m (linear) or NL x m NL (bilinear), column-major, NL = N (nw + 1): the
 *   loaded model of get_model / get_BLmodel.  Only the first nzeta rows of A and B are read (C = [I 0]).
 *   zeta: rows x nzeta, u: rows x m, column-major: the samples of every trial one after the other (already padded by the
 *   caller); trial_off (ntrials + 1): trial t owns rows trial_off[t] .. trial_off[t + 1] - 1.
 *   Window w covers rows s .. s + hor - 1 of trial win_trial[w], s = win_start[w] (trial-relative), and regresses the
 *   hor - 1 pairs k = s .. s + hor - 2:
 *     linear   rows A[:nz, :] kron(I_{nw+1}, psi(zeta_k)),                          right-hand side zeta_{k+1} - B[:nz, :] u_k
 *              (:1992-2004 with the undefined lift.Omega read as kron(I, econ_full), Kmpc.m:1320-1324)
 *     bilinear rows (A[:nz, :] + sum_j u_kj B_j[:nz, :]) kron(I_{nw+1}, psi(zeta_k)),  right-hand side zeta_{k+1}
 *              (the regression of Kmpc.m:1384-1394; :2003-2008 does not fit a bilinear B)
 *   and solves the lsqlin of :2021-2026: min ||R x - d||^2 over x = [1; w], -1 <= w <= 1; KP_OBS_RATE adds
 *   |w - whatpast_w| <= 0.01 (:2010-2019, whatpast: nwin x nw row-major, one previous estimate per window);
 *   KP_OBS_PIN_LAST pins the last load to zero (Kmpc.m:1350).  what (nwin x nw row-major), resnorm (nwin) =
 *   ||R x - d||^2 and status (nwin): KP_OK, or KP_ERR_QP_FAIL when the window's problem has no solution - a Hessian of the
 *   free loads that is not positive definite (fewer rows than free loads, or a Cholesky pivot below 1e-8 of its
 *   diagonal entry), a non-finite sample, an infeasible rate box - with what and resnorm NaN.
 *   Limits: 1 <= nw <= 8, 2 <= hor <= 1025; KP_ERR_ARG beyond them or for a window outside its trial.
 *   Three launches per call (lift, per-sample regression blocks, one wave per window) whatever the number of trials and
 *   windows, unless the rows the windows span need more than the call's fixed workspace: then per chunk of windows. */
int kp_load_observe(kp_ctx* ctx, const kp_basis* basis, int model_type, const double* A, const double* B, int nw,
                    int64_t rows, const double* zeta, const double* u, int ntrials, const int64_t* trial_off,
                    int64_t nwin, const int32_t* win_trial, const int64_t* win_start, int hor, const double* whatpast,
                    int flags, double* what, double* resnorm, int* status);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_OBSERVER_H */
