/* Prediction-horizon validation of a set of candidate models (kp_validate_horizon.hip): the companion of the validation table
 * of koopman_hip_validate.h, which includes this header, so a caller of kp_validate has it as well.  Like that header it is
 * kept apart from koopman_hip.h, whose entry points the MATLAB gateway matlab/kp_mex.c covers one for one. */
#ifndef KOOPMAN_HIP_HORIZON_H
#define KOOPMAN_HIP_HORIZON_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { KP_HORIZON_CHUNK = 8 };      /* horizon steps whose inputs and real outputs one workgroup of kp_validate_horizon stages at a time */

/* ---- prediction-horizon validation (kp_validate_horizon.hip): the h-step-ahead prediction errors, h = 1 .. H, from every
 * start sample of every trial - what a receding-horizon controller asks of a model, where kp_validate asks for one open-loop
 * rollout from row 0 over the whole trial ----
 * kp_validate_horizon: basis, model_type, N, m, n, nzeta, the nmod models A and B, trial_off, U and yfactor as kp_validate with
 *   nw = 0: unloaded models, discrete time.  Zeta: rows x nzeta, column-major over rows = trial_off[ntr]: the delay-embedded
 *   states zeta_0 .. zeta_{T-1} of every trial (get_zeta) after the nd shift; its first n columns are the real outputs y_j.
 *   Starts of trial q: s = 0, stride, 2 stride, ... while s + H <= T_q - 1, S_q of them (0 when T_q - 1 < H); every h is averaged
 *   over the same S_q starts.  Recursions (those of kp_validate):
 *     linear     z_0 = econ_full(zeta_s), z_{h+1} = A z_h + B u_{s+h}                 yhat_{s,h} = z_h(1:n)
 *     bilinear   z_{h+1} = A z_h + sum_i u_{s+h,i} B_i z_h
 *     nonlinear  zeta_0 = zeta_s, zeta_{h+1} = Kf econ_full([zeta_h; u_{s+h}])        yhat = zeta(1:n)
 *   err_out: nmod x ntr x H blocks of 2 n + 2, model-major, h = 1 .. H innermost: [mean |d| (n) | rmse (n) | euclid_mean |
 *   unscaled euclid_mean] over the S_q starts, d_{s,h} = yhat_{s,h} - y_{s+h}, the Euclidean norms over the outputs, the
 *   unscaled one of d .* yfactor (get_error, Ksysid.m:1886-1897; no nrmse: its normaliser belongs to a whole trial).
 *   nstart_out (ntr): S_q.  A trial with S_q = 0 gets NaN blocks.
 *   status_out (nmod x ntr): 1 when a prediction was not finite, else 0; such a pair's errors are what IEEE arithmetic gives,
 *   other pairs are untouched and the call returns KP_OK.
 *   One workgroup rolls a tile of S_T = 64, 32 or 16 consecutive starts of one trial with one model over the H steps; a step is
 *   a product of the model rows with the tile on the f64 matrix pipe.  S_T is the widest whose tiles fit 160 KB of LDS, per
 *   column of the tile: the start state (nvars + 2, up to a multiple of 4), with dim_red the full dictionary (nfull + 2), the
 *   operand (K + 2; K = N + m, N (1 + m) or N for a linear, bilinear or nonlinear model), the product (N + 2; nonlinear nzeta + 2)
 *   and KP_HORIZON_CHUNK (m + n + 2) staged inputs, outputs and norms.  It depends on the shape alone - never on nmod, ntr,
 *   the stride or the number of starts - and the sums over starts run in ascending order without atomics: every pair's numbers
 *   are the same bits alone or in any batch.  The model rows (padded to multiples of 4 each way) are staged in LDS when they fit
 *   beside the tiles, else read from memory.  kp_timer_get(24): the two kernels, ms; kp_timer_get(25): 1000 x (model staged) + S_T.
 *   KP_ERR_ARG, with a kp_last_error text: H < 1 or stride < 1; nmod < 1 or ntr < 1; a dictionary whose N, m, nzeta or model type
 *   is not the call's (so the bilinear dictionary of a loaded Ksysid) or whose columns are not econ_full's N; n > N or
 *   n > nzeta; NULL pointers; an empty trial; a shape whose tiles do not fit the LDS at S_T = 16. */
int kp_validate_horizon(kp_ctx* ctx, const kp_basis* basis, int model_type, int N, int m, int n, int nzeta, int nmod,
                        const double* A, const double* B, int ntr, const int64_t* trial_off, const double* Zeta,
                        const double* U, const double* yfactor, int H, int stride,
                        double* err_out, int64_t* nstart_out, int* status_out);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_HORIZON_H */
