/* The validation table of a set of candidate models (kp_validate.hip).  Kept apart from koopman_hip.h, whose entry points
 * the MATLAB gateway matlab/kp_mex.c covers one for one: MATLAB keeps the reference's valNplot_model, this is for C and
 * Python callers. */
#ifndef KOOPMAN_HIP_VALIDATE_H
#define KOOPMAN_HIP_VALIDATE_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KP_VALIDATE_CHUNK = 128 };   /* time steps whose inputs, loads and outputs one workgroup stages at a time */

/* ---- validation table (replaces the loop of valNplot_model, Ksysid.m:1928-1972, over val_model :1623-1714, val_BLmodel
 * :1717-1812 or val_NLmodel :1815-1879 and get_error :1882-1898, for every candidate of a lasso grid) ----
 * kp_validate: nmod models rolled out over ntr trials, nmod x ntr rollouts in one launch, the errors reduced on the device.
 *   basis: the UNLOADED dictionary of the model type (psi = econ_full; N, m and nzeta must be its own), model_type
 *   KP_MODEL_LINEAR, KP_MODEL_BILINEAR or KP_MODEL_NONLINEAR, discrete time.  n <= N outputs (nonlinear: n <= nzeta),
 *   nw >= 0 loads, NL = N (nw + 1).
 *   A: nmod matrices back to back, column-major: NL x NL (linear, bilinear: A of get_model / get_BLmodel) or nzeta x NL
 *   (nonlinear: Kf of get_NLmodel).  B: nmod matrices NL x m (linear) or NL x m NL (bilinear); NULL for nonlinear.
 *   Trial q owns rows trial_off[q] .. trial_off[q + 1] - 1 (its T_q >= 1 rows after the nd shift) of U (rows x m), Yreal
 *   (rows x n) and Wl (rows x nw; NULL when nw = 0), all column-major over rows = trial_off[ntr]; zeta0: ntr x nzeta
 *   column-major, the first delay-embedded state of each trial.  yfactor (n): the factors of scaleup.y.
 *   Recursions, with wt_j = [1; w_j] the load of step j (a loaded model weights its nw + 1 column blocks of N by it,
 *   znow = kron(I, z(1:N)) wt_j, and only rows 1:N feed forward; :1667-1668, :1761, :1857):
 *     linear     z+ = sum_l wt_l A(1:N, block l) z + B(1:N, :) u_j                             z_0 = econ_full(zeta0)
 *     bilinear   z+ = sum_l wt_l A(1:N, block l) z + sum_i u_ji sum_l wt_l B_i(1:N, block l) z
 *     nonlinear  zeta+ = sum_l wt_l Kf(:, block l) econ_full([zeta; u_j])                     zeta_0 = zeta0
 *   ysim = the first n entries of the state; row 0 of ysim is row 0 of Yreal (:1654).
 *   err_out: nmod x ntr blocks of 3 n + 2, model-major: [mean |d| (n) | rmse (n) | nrmse (n) | euclid_mean |
 *   unscaled euclid_mean], d = ysim - yreal, sums over the T_q rows divided by T_q, nrmse = rmse / |max - min| of yreal,
 *   the unscaled distance that of d .* yfactor (:1886-1897).  A trial of one row gives zeros and nrmse = NaN.
 *   status_out (nmod x ntr): 1 when a simulated output was not finite, else 0; such a pair's errors are the Inf / NaN IEEE
 *   arithmetic gives, and the call still returns KP_OK.
 *   Ysim (want_sim != 0; else it may be NULL): nmod blocks of rows x n, column-major.
 *   Every pair's numbers depend on that pair alone: they are the same bits alone or in any batch.
 *   Limits (KP_ERR_ARG): the state vectors, the error sums and one chunk of KP_VALIDATE_CHUNK steps - (m + nw + 2 n + 2)
 *   doubles per step - must fit 160 KB of LDS; a model that fits beside them is staged there, a larger one is read from
 *   memory. */
int kp_validate(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nw, int nmod,
                const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0, const double* U,
                const double* Yreal, const double* Wl, const double* yfactor, int want_sim, double* err_out,
                int* status_out, double* Ysim);

enum {
  KP_VALIDATE_CT_CHUNK = 32,     /* samples whose inputs and outputs one workgroup of kp_validate_ct stages at a time */
  KP_VALIDATE_CT_STAGE = 8192    /* doubles of A, Kf or the bilinear A + sum_i u_i B_i that kp_validate_ct keeps in LDS */
};

/* ---- validation table of continuous-time models (kp_validate_ct.hip; the same loop over val_model :1679-1683, val_BLmodel
 * :1777-1781 or val_NLmodel :1849-1856 with time_type = 'continuous') ----
 * kp_validate_ct: kp_validate for models of z' = A z + B u_j (linear), z' = (A + sum_i u_ji B_i) z (bilinear) or
 *   zeta' = Kf econ_full([zeta; u_j]) (nonlinear, lifted in the kernel at every stage): every sample interval is integrated
 *   over [0, Ts] with the input of row j held, from the end point of the previous one, by ode45's Dormand-Prince 5(4) pair
 *   with the step control of kp_rollout_ct / kp_rollout_nl_ct (koopman_hip_ct.h; rtol = RelTol, atol = AbsTol).
 *   basis, model_type, N, m, n, nzeta, the models A and B, trial_off, zeta0, U, Yreal, yfactor, want_sim, err_out and Ysim:
 *   as kp_validate.  nw must be 0 and Wl is not read (Ksysid refuses loaded continuous-time models).
 *   ysim = the first n entries of the state; row 0 of ysim is row 0 of Yreal (:1654).
 *   A failed integration (step-size underflow, more than 100000 steps in one interval, a non-finite state) is data, not an
 *   error: the samples from the failing one on are NaN, status_out (nmod x ntr) is 1 - as it is whenever a simulated output
 *   is not finite - the pair's errors are what IEEE arithmetic gives, and the call returns KP_OK.
 *   naccept / nreject (nmod x ntr, may be NULL): accepted / rejected steps over the whole rollout of a pair.
 *   Every pair's numbers depend on that pair alone: they are the same bits alone or in any batch.
 *   Limits (KP_ERR_ARG): nw != 0; Ts, rtol or atol not positive and finite; N > 512; n > N (nonlinear: n > nzeta); 11 state
 *   and stage vectors, the error sums, one chunk of KP_VALIDATE_CT_CHUNK samples - (m + 2 n + 2) doubles per sample - and
 *   B u (N) or, for a nonlinear model, the dictionary scratch (nvars + nfull + N) must fit 160 KB of LDS.  A matrix of at
 *   most KP_VALIDATE_CT_STAGE doubles that fits beside them is staged there; a larger A or Kf is read from memory, a larger
 *   bilinear A + sum_i u_i B_i lives in a per-pair slice of device scratch (nmod ntr N N doubles). */
int kp_validate_ct(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nw, int nmod,
                   const double* A, const double* B, int ntr, const int64_t* trial_off, const double* zeta0, const double* U,
                   const double* Yreal, const double* Wl, const double* yfactor, int want_sim, double Ts, double rtol,
                   double atol, double* err_out, int* status_out, double* Ysim, int* naccept, int* nreject);

#ifdef __cplusplus
}
#endif

/* prediction-horizon validation, the h-step-ahead errors from every start sample (kp_validate_horizon): its own header */
#include "koopman_hip_horizon.h"
#endif /* KOOPMAN_HIP_VALIDATE_H */
