/* Whole closed loops with the identified model as the plant (kp_mpc.hip).  Kept apart from koopman_hip.h, whose entry
 * points the MATLAB gateway matlab/kp_mex.c covers one for one: MATLAB keeps its own run_simulation loop, this is for C and
 * Python callers. */
#ifndef KOOPMAN_HIP_SIM_H
#define KOOPMAN_HIP_SIM_H
#include "koopman_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- batched closed loops (replaces the loop of Kmpc.run_simulation, Kmpc.m:403-512, for nb trials at once) ----
 * kp_mpc_simulate: nb independent closed loops of one controller in ONE launch, one workgroup per trial, everything in
 *   scaled units.  For k = 1 .. nref-1 a trial lifts zeta = Y[k-1] (the fused lift of kp_mpc_step_zeta), runs the step of
 *   kp_mpc_step (iters as there) against rows k-1 .. k-1+Np of its reference - the last row repeated behind the end,
 *   Kmpc.m:354-365 and :473-477 - with u_prev = U[k-1], sets U[k] to the second row of the solution and
 *   Y[k] = (A z + B u_prev)[0:n] (linear) or (A z + sum_i u_prev,i B_i z)[0:n] (bilinear): the one-step input delay of
 *   Kmpc.m:495-496 with C = [I 0].  Each trial warm-starts a step from its OWN previous active set; the state of the loop
 *   stays in LDS.  A trial's result does not depend on nb or on its index.
 *   n is the dictionary's nzeta: the loop is the reference's, delays = 0.  The dictionary of a model with delays has
 *   nzeta = n (nd + 1) + m nd and would be read as that many outputs - a caller that knows n must refuse it (Mpc.simulate
 *   does).
 *   ref: [nb][nref][nproj] row-major, or one [nref][nproj] block for every trial with ref_shared != 0; y0 [nb][n],
 *   u0 [nb][m].  U [nb][nref][m] and Y [nb][nref][n]: row 0 = u0 / y0.  Z ([nb][nref-1][N], may be NULL): row k-1 = the
 *   lifted state of step k.  steps_done[i]: the steps trial i completed; status[i]: KP_OK or KP_ERR_QP_FAIL.
 *   A failed QP at step k ends THAT trial (the break of Kmpc.m:483-485): steps_done = k-1, rows k.. of U and Y and rows
 *   k-1.. of Z are NaN; the call still returns KP_OK.  nref = 1 runs no step and writes row 0.
 *   KP_ERR_ARG: nb < 1, nref < 1 or iters < 1; a dictionary whose N is not the controller's (a loaded controller among
 *   them); a controller with state bounds (those steps go through the generic QP kernel); horizon < 2; a shape whose step
 *   plus the reference of nref + Np rows exceeds the 160 KB of LDS.  The model's P | PB block is staged in LDS once per
 *   trial when it still fits, else read from L2.
 *   Inputs and outputs cross in one copy each up to 4 MB in total; beyond, the outputs are copied to the caller's arrays
 *   directly.  kp_timer_get(19): the kernel, ms. */
int kp_mpc_simulate(kp_mpc* mpc, const kp_basis* basis, int nb, int nref, const double* ref, int ref_shared,
                    const double* y0, const double* u0, int iters, double* U, double* Y, double* Z, int* steps_done,
                    int* status);

#ifdef __cplusplus
}
#endif
#endif /* KOOPMAN_HIP_SIM_H */
