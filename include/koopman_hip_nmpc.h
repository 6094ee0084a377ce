/* Nonlinear MPC entry points of libkoopman_hip.so (kp_nmpc.hip).  Kept apart from koopman_hip.h, whose entry points the
 * MATLAB gateway matlab/kp_mex.c covers one for one: MATLAB keeps fmincon for nonlinear MPC (KmpcHip.m), these are for C
 * and Python callers. */
#ifndef KOOPMAN_HIP_NMPC_H
#define KOOPMAN_HIP_NMPC_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kp_nmpc kp_nmpc;           /* nonlinear MPC (SQP) problem on device */

/* ---- nonlinear MPC (replaces Kmpc.get_mpcInput_nonlinear and its fmincon SQP, Kmpc.m:906-1181) ----
 * kp_lift_jacobian: d econ_full / dv at nrows points V (nrows x nvars column-major; v = [zeta; u] for a nonlinear
 *   dictionary, zeta otherwise): J holds per row an N x nvars column-major block (row r at J + r N nvars).  Every column
 *   kind of the dictionary (variables, monomials, hermite, fourier, fourier_sparser, gaussian); with dim_red the rows
 *   are [I; pcs' dfull/dv; 0] (Ksysid.m:1615-1618).  KP_ERR_ARG when nvars + nfull * nvars (nvars
 *   rounded up to even) exceeds 8192 doubles.
 * kp_nmpc_create: get_costMatrices_nonlinear / get_constraintMatrices_nonlinear (Kmpc.m:909-1059) for the model
 *   F(zeta, u) = Kf econ_full([zeta; u]) (get_NLmodel, Ksysid.m:1298-1341): basis must be a nonlinear dictionary, Kf is
 *   nzeta x N column-major, proj nproj x nzeta (projmtx(:, 1:n)), r the diagonal of R (m), lo / hi the scaled-down input
 *   bounds on all Np inputs (NULL: none), slope_lim / smooth_lim already scaled (NaN: none; the smooth rows use -2 I for the
 *   reference's -2*Fslope_i).  KP_ERR_ARG when m*Np > 64 or the step's workspace exceeds the 160 KB of LDS.
 * kp_nmpc_set_state_bounds: scaled-down bounds lo <= z_k <= hi on all n = nzeta states of every z_k, k = 0..Np
 *   (Kmpc.m:1036-1052: these rows stride by n); n = 0 removes them.
 * kp_nmpc_set_options: SQP iteration cap (default 60), the tolerances of the stopping test on the KKT residual and the
 *   step (default 1e-8 each) and the initial Levenberg-Marquardt damping nu of the QP Hessian, Hq + nu diag(Hq) (default
 *   10; 0: plain Gauss-Newton).
 * kp_nmpc_step: one get_mpcInput_nonlinear call.  zeta (nzeta), u_prev = traj.u(end,:) (m), Yr the padded, vectorised
 *   reference (nproj (Np+1)), U_init: NULL for the reference's start X0 (u_prev repeated, :1155) or an Np x m column-major
 *   first iterate (its first row is replaced by u_prev).  U_out: Np x m column-major, row 1 = u_prev.  Z_out ((Np+1) x nzeta
 *   row-major per state, may be NULL): z_0 .. z_Np of the returned inputs.  info (2, may be NULL): SQP iterations, KKT
 *   residual.  *status: KP_OK; KP_ERR_QP_FAIL (infeasible or failed QP subproblem: U_out NaN); KP_ERR_NOT_CONVERGED
 *   (iteration cap or no decrease along the step: the last iterate).
 * kp_nmpc_step_batch: nb independent problems of the same controller, every array per problem contiguous; the same
 *   kernel as kp_nmpc_step (its nb = 1 case).
 * kp_nmpc_simulate: nb closed loops with the model itself as the plant (Kmpc.run_simulation, Kmpc.m:403-512) in one launch,
 *   one workgroup per trial, everything in scaled units.  ref: [nb][nref][nproj] row-major, or one block for all trials
 *   with ref_shared != 0; y0 [nb][nzeta], u0 [nb][m].  Step k = 1 .. nref-1 of a trial is the SQP of kp_nmpc_step (the
 *   controller's options; mu and the damping restart at every step) at zeta = Y[k-1], u_prev = U[k-1] against reference rows
 *   k-1 .. k-1+Np (the last row repeated behind the end); then U[k] = row 2 of its solution and Y[k] = F(Y[k-1], U[k-1]), the
 *   one-step input delay of :495-496.  The start of a step is X0 (u_prev repeated); with warm != 0 and k > 1 the previous
 *   step's returned inputs shifted by one row, last row repeated, row 1 = u_prev.  U [nb][nref][m], Y [nb][nref][nzeta], row 0
 *   = u0 / y0; info ([nb][nref-1][3], may be NULL): SQP iterations, KKT residual, status of every step.  A step that ends
 *   KP_ERR_NOT_CONVERGED returns its last iterate and the trial goes on; a failed QP subproblem ends that trial only:
 *   steps_done[i] = k-1, rows k.. of U and Y and the info rows from that step on are NaN.  status[i]: KP_ERR_QP_FAIL (ended
 *   early), KP_ERR_NOT_CONVERGED (completed with at least one unconverged step), else KP_OK; the call returns KP_OK whatever
 *   the trials did.  nref = 1 writes row 0 and runs no step.  State bounds (kp_nmpc_set_state_bounds) hold in the loop.  A
 *   trial's result does not depend on nb or on its index, bit for bit.  KP_ERR_ARG: nb < 1, nref < 1, a NULL pointer other
 *   than info, horizon < 2, or the step's workspace plus the staged reference ((nref + Np) nproj doubles) beyond the 160 KB
 *   of LDS.  kp_timer_get(21): the kernel, ms.
 * kp_nmpc_last_jacobians: [A_k B_k] = dF/d[zeta; u] at the Np points of the last linearisation of the last single step
 *   (Np blocks of nzeta x nvars, column-major). */
int kp_lift_jacobian(kp_ctx* ctx, const kp_basis* basis, int nrows, const double* V, double* J);
int kp_nmpc_create(kp_ctx* ctx, const kp_basis* basis, const double* Kf, int Np, const double* proj, int nproj,
                   double q_run, double q_term, const double* r, const double* lo, const double* hi, double slope_lim,
                   double smooth_lim, kp_nmpc** nmpc);
int kp_nmpc_set_state_bounds(kp_nmpc* nmpc, int n, const double* lo, const double* hi);
int kp_nmpc_set_options(kp_nmpc* nmpc, int max_iter, double tol_kkt, double tol_step, double damping);
int kp_nmpc_dims(const kp_nmpc* nmpc, int* nvar, int* nrows);
int kp_nmpc_step(kp_nmpc* nmpc, const double* zeta, const double* u_prev, const double* Yr, const double* U_init,
                 double* U_out, double* Z_out, double* info, int* status);
int kp_nmpc_step_batch(kp_nmpc* nmpc, int nb, const double* zeta, const double* u_prev, const double* Yr,
                       const double* U_init, double* U_out, double* Z_out, double* info, int* status);
int kp_nmpc_simulate(kp_nmpc* nmpc, int nb, int nref, const double* ref, int ref_shared, const double* y0, const double* u0,
                     int warm, double* U, double* Y, double* info, int* steps_done, int* status);
int kp_nmpc_last_jacobians(kp_nmpc* nmpc, double* J);
int kp_nmpc_destroy(kp_nmpc* nmpc);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_NMPC_H */
