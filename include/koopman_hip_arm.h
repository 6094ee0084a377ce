/* The planar arm plant (kp_arm.hip): batched ode45 simulation of the reference's Arm class.  Kept apart from
 * koopman_hip.h, whose entry points the MATLAB gateway matlab/kp_mex.c covers one for one: this serves Python and C
 * callers that generate training data or step the plant of a closed loop. */
#ifndef KOOPMAN_HIP_ARM_H
#define KOOPMAN_HIP_ARM_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Physical parameters of Arm.m's params struct: Nmods modules of nlinks links each (Nlinks = Nmods nlinks), link
 * length l, joint stiffness k, damping d, link mass m, link inertia i, gravity g, input stiffness ku. */
typedef struct {
  int Nmods, nlinks;
  double l, k, d, m, i, g, ku;
} kp_arm_params;

/* Modes of kp_arm_simulate.  Rows are 0-based; s is the stage time of the integrator; row r of U / W is the input /
 * load of sample r; T_out is the number of output rows.
 *   KP_ARM_SPAN_ZOH     Arm.simulate(t, u, w) with input_type 'zoh' (Arm.m:1004): ONE integration over [t_0, t_{T-1}],
 *                       T_out = T, output at every t_j.  Input and load row: get_k (Arm.m:1044-1052), i.e. row 1 at
 *                       s = 0 and row j + 1 for s in (t_j, t_{j+1}] (clamped to T - 1).
 *   KP_ARM_SPAN_INTERP  input_type 'interp' (Arm.m:1005-1009): ONE integration over [t_0, t_{T-2}], T_out = T - 1.
 *                       With j as above (j = 0 at s = 0), r = j + 1: u(s) = U_r + (U_{r+1} - U_r) / (t_{r+1} - t_r) (s - t_r)
 *                       (an extrapolation back from t_r on (t_j, t_r]); load row r, not interpolated.  T >= 3.
 *   KP_ARM_SPAN_FLOOR   simulate_rampNhold (Arm.m:900): ONE integration over [t_0, t_{T-1}], T_out = T, input and load
 *                       row floor(s / Ts) (IEEE division, clamped to [0, T - 1]).  The reference's load is constant.
 *   KP_ARM_RESTART      Arm.simulate_Ts per sample (Arm.m:932-957): X_0 = x0 and X_{j+1} = ode45 over [0, t_{j+1} - t_j]
 *                       from X_j with input and load row j held.  T_out = T.
 * Every integration is ode45's Dormand-Prince 5(4) pair with its step control as arm.dopri45 / arm.ode45_span restate
 * it: MaxStep 0.1 (span), initial trial step min(MaxStep, t_1 - t_0) (the first interval of the span), the 1.1 h stretch
 * to the end point, shrink by max(0.1, 0.8 (rtol / err)^(1/5)) on the first failure of a step and by 1/2 after,
 * growth of at most 5x.  Span outputs are the step end where a step ends on t_j, else ntrp45's interpolant. */
enum { KP_ARM_SPAN_ZOH = 0, KP_ARM_SPAN_INTERP = 1, KP_ARM_SPAN_FLOOR = 2, KP_ARM_RESTART = 3 };

/* kp_arm_simulate: `batch` trials in one launch, one GPU lane per trial.
 *   t (T): the shared time vector, t_0 = 0 and strictly increasing.  Ts: the sampling period of KP_ARM_SPAN_FLOOR
 *   (ignored otherwise).  x0 (batch x 2 Nlinks, NULL: rest).  U (batch x T x Nmods).  W (batch x T x 2: end-effector
 *   mass and gravity angle, NULL: no load).  X out (batch x T_out x 2 Nlinks, [alpha, alphadot]).  All row-major.
 *   naccept / nreject (batch, may be NULL): accepted / rejected steps of the trial.
 *   status (batch): KP_OK, or KP_ERR_NOT_CONVERGED for a step-size underflow, more than 100000 attempted steps between
 *   two outputs or a non-finite state; that trial's rows from the first output not reached are NaN.  The other trials
 *   are not affected: each trial's result does not depend on the batch around it.
 *   Returns KP_ERR_ARG (kp_last_error says why) for 1 > Nlinks or Nlinks > 8, Nmods or nlinks < 1, T < 2 (T < 3 for
 *   KP_ARM_SPAN_INTERP), t not starting at 0 or not strictly increasing, rtol / atol (or Ts in KP_ARM_SPAN_FLOOR) not
 *   positive and finite, non-finite params, an unknown mode or a NULL t / U / X / status. */
int kp_arm_simulate(kp_ctx* ctx, const kp_arm_params* params, int mode, int batch, int T, const double* t, double Ts,
                    const double* x0, const double* U, const double* W, double rtol, double atol, double* X, int* naccept,
                    int* nreject, int* status);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_ARM_H */
