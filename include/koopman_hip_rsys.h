/* The random-system generator (kp_rsys.hip): batched ode45 simulation of the reference's Rsys trials.  Kept apart from
 * koopman_hip.h, whose entry points the MATLAB gateway matlab/kp_mex.c covers one for one: this serves Python and C
 * callers that generate the data of the random-system sweep (evaluate_rand_models.m). */
#ifndef KOOPMAN_HIP_RSYS_H
#define KOOPMAN_HIP_RSYS_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The shape shared by every system of a set (Rsys.m:34-91): num_terms monomial terms, x^a u^b with a <= degree_x and
 * b <= degree_u.  System i is xdot = exp(-x^4) (sum_j c_ij x^(a_ij) u^(b_ij) + c_u,i u) - atan(x). */
typedef struct {
  int num_terms, degree_x, degree_u;
} kp_rsys_dims;

/* Modes of kp_rsys_simulate.  Rows are 0-based; s is the stage time of the integrator; row r of a trial's inputs is the
 * input of sample r.
 *   KP_RSYS_SPAN     Rsys.simulate_systems (Rsys.m:118): ONE ode45 over [t_0, t_{T-1}].  The input of stage time s is
 *                    row j = the last index with t_j <= s (get_u, Rsys.m:128-133), clamped to [0, T - 1].  MaxStep is
 *                    0.1 (t_{T-1} - t_0), the initial trial step min(MaxStep, t_1 - t_0).  The output at t_j is the step
 *                    end where a step ends on t_j, else ntrp45's interpolant.
 *   KP_RSYS_RESTART  rsys.py's host mirror: Y_0 = x0 and Y_{k+1} = ode45 over [t_k, t_{k+1}] from Y_k with row k held,
 *                    MaxStep 0.1 (t_{k+1} - t_k); a step that reaches t_{k+1} ends exactly on it.
 * Every integration is ode45's Dormand-Prince 5(4) pair with its step control as arm.dopri45 / arm.ode45_span restate
 * it: the 1.1 h stretch to the end point, hmin = 16 eps |t|, shrink by max(0.1, 0.8 (rtol / err)^(1/5)) on the first
 * failure of a step and by 1/2 after, growth of at most 5x. */
enum { KP_RSYS_SPAN = 0, KP_RSYS_RESTART = 1 };

/* kp_rsys_simulate: nsys x ntrials trials in one launch, one GPU lane per (system, trial), system-major.
 *   t (T): the shared time vector, t_0 = 0 and strictly increasing.
 *   coeffs, pow_x, pow_u (nsys x num_terms): c_ij, a_ij, b_ij.  input_gain (nsys): c_u,i.  x0 (ntrials): the initial
 *   state of trial j, shared by all systems (Rsys.m:104-106).
 *   U, chosen by hold: hold == 0, nsys x ntrials x T (every row); hold >= 1, nsys x ntrials x nlev with
 *   nlev = ceil(T / hold), the levels of generate_input_steps (Rsys.m:136-150): row r takes level r / hold for
 *   r < hold (nlev - 1) and 0 after that (the reference's zero tail; its last level is drawn but never used).
 *   Y out (nsys x ntrials x T, may be NULL).  naccept / nreject (nsys x ntrials, may be NULL): accepted / rejected steps.
 *   status (nsys x ntrials): KP_OK, or KP_ERR_NOT_CONVERGED for a step-size underflow, more than 100000 attempted steps
 *   between two outputs or a non-finite state; that trial's rows from the first output not reached are NaN.  The other
 *   trials are not affected: each trial's result does not depend on the batch around it.  All arrays row-major.
 *   traj (may be NULL): also create a finished kp_traj in the layout of Rsys.save_data (Rsys.m:182-216): trials
 *   0 .. ntrials-2 of every system merged as training data, trial ntrials-1 as the validation trial, n = m = 1, the
 *   scaling computed on the device; the data never leaves it.  If any trial failed, no object is created and the call
 *   returns KP_ERR_NOT_CONVERGED (the host outputs are still written).
 *   Returns KP_ERR_ARG (kp_last_error says why) for nsys or num_terms < 1, ntrials < 1 (< 2 with traj), T < 3,
 *   degree_x or degree_u outside 0..15, a power outside 0..degree, t not starting at 0 or not strictly increasing,
 *   rtol / atol not positive and finite, an unknown mode, a negative hold or a NULL t / coeffs / pow_x / pow_u /
 *   input_gain / x0 / U / status. */
int kp_rsys_simulate(kp_ctx* ctx, const kp_rsys_dims* dims, int mode, int nsys, int ntrials, int T, const double* t,
                     const double* coeffs, const int* pow_x, const int* pow_u, const double* input_gain, const double* x0,
                     const double* U, int hold, double rtol, double atol, double* Y, int* naccept, int* nreject,
                     int* status, kp_traj** traj);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_RSYS_H */
