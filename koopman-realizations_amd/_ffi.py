"""ctypes binding of libkoopman_hip.so (the C ABI declared in include/koopman_hip.h).

The library is the product; there is no CPU fallback.  If the shared object is missing
or cannot be loaded this module raises, and every compute call fails loudly when no HIP
device is present (kp_create returns KP_ERR_HIP).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KP_LIB_PATH") or os.path.join(_HERE, "libkoopman_hip.so")     # KP_LIB_PATH: an experimental build (tools/)

KP_OK, KP_ERR_ARG, KP_ERR_HIP, KP_ERR_NOT_SPD, KP_ERR_QP_FAIL, KP_ERR_NOT_CONVERGED = 0, -1, -2, -3, -4, -5
MODEL = {"linear": 0, "bilinear": 1, "nonlinear": 2}
BLOCK = {"poly": 0, "fourier": 1, "gaussian": 2, "hermite": 3, "fourier_sparser": 4}
LIFT_FULL, LIFT_ECON, LIFT_ROW = 0, 1, 2

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int)
vp = C.c_void_p


class KpBasisDesc(C.Structure):
    _fields_ = [("model_type", C.c_int32), ("nzeta", C.c_int32), ("m", C.c_int32), ("n_blocks", C.c_int32),
                ("block_type", C.POINTER(C.c_int32)), ("block_count", C.POINTER(C.c_int32)),
                ("poly_exps", C.POINTER(C.c_uint8)), ("gauss_centres", c_dp),
                ("k_pcs", C.c_int32), ("pcs", c_dp)]


# name -> (restype, argtypes); every symbol of include/koopman_hip.h
SIGNATURES = {
    "kp_device_count": (C.c_int, [c_ip]),
    "kp_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
    "kp_destroy": (C.c_int, [vp]),
    "kp_last_error": (C.c_char_p, [vp]),
    "kp_device_info": (C.c_int, [vp, C.c_char_p, C.c_int, c_ip, C.POINTER(C.c_int64)]),
    "kp_timer_get": (C.c_int, [vp, C.c_int, c_dp]),
    "kp_stream": (vp, [vp]),
    "kp_basis_create": (C.c_int, [vp, C.POINTER(KpBasisDesc), C.POINTER(vp)]),
    "kp_basis_destroy": (C.c_int, [vp]),
    "kp_basis_dims": (C.c_int, [vp, c_ip, c_ip, c_ip, c_ip]),
    "kp_basis_desc_dims": (C.c_int, [C.POINTER(KpBasisDesc), c_ip, c_ip, c_ip, c_ip]),
    "kp_lift": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp, C.c_int64, c_dp]),
    "kp_snapshots_upload": (C.c_int, [vp, c_dp, c_dp, c_dp, C.c_int64, C.c_int, C.c_int, C.POINTER(vp)]),
    "kp_snapshots_update": (C.c_int, [vp, vp, c_dp, c_dp, c_dp, C.c_int64]),
    "kp_snapshots_destroy": (C.c_int, [vp]),
    "kp_host_alloc": (C.c_int, [vp, C.c_int64, C.POINTER(vp)]),
    "kp_host_free": (C.c_int, [vp, vp]),
    "kp_fit_gram": (C.c_int, [vp, vp, vp, c_dp, c_dp]),
    "kp_fit_solve": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, c_dp]),
    "kp_fit_last_rank": (C.c_int, [vp, c_ip]),
    "kp_fit_last_pivot_ratio": (C.c_int, [vp, c_dp]),
    "kp_fit_lasso": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double, c_dp, c_ip]),
    "kp_fit_lasso_batch": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, c_dp, C.c_int, C.c_int, C.c_double, c_dp, c_ip]),
    "kp_fit": (C.c_int, [vp, vp, vp, c_dp, C.c_int, c_dp]),
    "kp_synchronize": (C.c_int, [vp]),
    "kp_fit_async_slots": (C.c_int, [vp, C.c_int]),
    "kp_fit_get_K": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "kp_fit_batch": (C.c_int, [vp, vp, vp, C.c_int, C.c_int64, c_dp, c_dp, c_dp, C.POINTER(C.c_int)]),
    "kp_traj_upload": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.POINTER(vp)]),
    "kp_traj_destroy": (C.c_int, [vp]),
    "kp_traj_create": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]),
    "kp_traj_put": (C.c_int, [vp, C.c_int, c_dp]),
    "kp_traj_finish": (C.c_int, [vp]),
    "kp_traj_scale": (C.c_int, [vp, c_dp]),
    "kp_traj_dims": (C.c_int, [vp, c_ip, c_ip, c_ip, c_ip, c_ip, c_ip]),
    "kp_sweep_eval": (C.c_int, [vp, vp, vp, C.c_double, c_dp, c_dp, c_ip]),
    "kp_sweep_eval_nested": (C.c_int, [vp, vp, vp, C.c_double, C.c_int, c_dp, c_ip]),
    "kp_sweep_nested_get_K": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp]),
    "kp_fit_refine": (C.c_int, [vp, vp, vp, C.c_int, c_dp]),
    "kp_sym_eig": (C.c_int, [vp, c_dp, C.c_int, c_dp, c_dp, C.POINTER(C.c_int)]),
    "kp_mpc_set_state_bounds": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "kp_model_project_batch": (C.c_int, [vp, c_dp, c_dp, c_dp, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_dp, C.POINTER(C.c_int)]),
    "kp_model_project": (C.c_int, [vp, c_dp, c_dp, c_dp, C.c_int, C.c_int, c_dp, c_dp, c_dp]),
    "kp_rollout": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, c_dp]),
    "kp_rollout_nl": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_dp]),
    "kp_mpc_create": (C.c_int, [vp, C.c_int, c_dp, c_dp, C.c_int, C.c_int, C.c_int, c_dp, C.c_int, C.c_double,
                                C.c_double, c_dp, c_dp, c_dp, C.c_double, C.c_double, C.POINTER(vp)]),
    "kp_mpc_destroy": (C.c_int, [vp]),
    "kp_mpc_dims": (C.c_int, [vp, c_ip, c_ip]),
    "kp_mpc_step": (C.c_int, [vp, c_dp, c_dp, c_dp, C.c_int, c_dp, c_ip]),
    "kp_mpc_step_zeta": (C.c_int, [vp, vp, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp, c_ip]),
    "kp_mpc_step_batch": (C.c_int, [vp, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "kp_mpc_step_loaded": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, C.c_int, c_dp, c_dp,
                                     c_dp, c_dp, c_ip]),
    "kp_mpc_last_qp": (C.c_int, [vp, c_dp, c_dp, c_dp, c_dp]),
    "kp_mpc_last_profile": (C.c_int, [vp, c_dp, c_ip]),
    "kp_mpc_last_stamps": (C.c_int, [vp, c_dp]),
    "kp_qp_solve": (C.c_int, [vp, c_dp, c_dp, c_dp, c_dp, C.c_int, C.c_int, c_dp, c_ip]),
    "kp_comm_unique_id": (C.c_int, [vp]),
    "kp_comm_create": (C.c_int, [vp, vp, C.c_int, C.c_int]),
    "kp_comm_destroy": (C.c_int, [vp]),
    "kp_comm_info": (C.c_int, [vp, c_ip, c_ip]),
    "kp_comm_allgather": (C.c_int, [vp, vp, C.c_int64, vp]),
    "kp_comm_allreduce_sum": (C.c_int, [vp, c_dp, C.c_int64]),
    "kp_comm_abandon": (C.c_int, [vp]),
    "kp_comm_allgather_fit": (C.c_int, [vp, C.c_int, C.c_int, c_dp]),
    "kp_comm_allgather_fits": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, c_dp]),
    "kp_comm_gather_fits": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, c_dp]),
    "kp_fit_sharded": (C.c_int, [vp, vp, vp, c_dp, C.c_int, c_dp]),
    "kp_fit_gram_sharded": (C.c_int, [vp, vp, vp, c_dp, c_dp]),
    "kp_multi_create": (C.c_int, [c_ip, C.c_int, C.POINTER(vp)]),
    "kp_multi_destroy": (C.c_int, [vp]),
    "kp_multi_size": (C.c_int, [vp, c_ip]),
    "kp_multi_ctx": (vp, [vp, C.c_int]),
    "kp_multi_last_error": (C.c_char_p, [vp]),
    "kp_multi_host_alloc": (C.c_int, [vp, C.c_int64, C.POINTER(vp)]),
    "kp_multi_host_free": (C.c_int, [vp, vp]),
    "kp_multi_timers": (C.c_int, [vp, c_dp]),
    "kp_multi_fit": (C.c_int, [vp, C.POINTER(KpBasisDesc), c_dp, c_dp, c_dp, C.c_int64, c_dp, C.c_int, c_dp]),
    "kp_multi_fit_sharded": (C.c_int, [vp, C.POINTER(KpBasisDesc), c_dp, c_dp, c_dp, C.c_int64, c_dp, C.c_int, c_dp]),
    "kp_multi_traj_upload": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.POINTER(vp)]),
    "kp_multi_traj_destroy": (C.c_int, [vp]),
    "kp_multi_sweep_eval_nested": (C.c_int, [vp, vp, C.POINTER(KpBasisDesc), C.c_double, C.c_int, c_dp, c_ip]),
    "kp_multi_mpc_create": (C.c_int, [vp, C.c_int, c_dp, c_dp, C.c_int, C.c_int, C.c_int, c_dp, C.c_int, C.c_double,
                                      C.c_double, c_dp, c_dp, c_dp, C.c_double, C.c_double, C.POINTER(vp)]),
    "kp_multi_mpc_set_state_bounds": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "kp_multi_mpc_destroy": (C.c_int, [vp]),
    "kp_multi_mpc_step_batch": (C.c_int, [vp, C.c_int, c_dp, c_dp, c_dp, c_dp, c_ip]),
}

# the nonlinear MPC entry points (include/koopman_hip_nmpc.h)
NMPC_SIGNATURES = {
    "kp_lift_jacobian": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp]),
    "kp_nmpc_create": (C.c_int, [vp, vp, c_dp, C.c_int, c_dp, C.c_int, C.c_double, C.c_double, c_dp, c_dp, c_dp,
                                 C.c_double, C.c_double, C.POINTER(vp)]),
    "kp_nmpc_set_state_bounds": (C.c_int, [vp, C.c_int, c_dp, c_dp]),
    "kp_nmpc_set_options": (C.c_int, [vp, C.c_int, C.c_double, C.c_double, C.c_double]),
    "kp_nmpc_dims": (C.c_int, [vp, c_ip, c_ip]),
    "kp_nmpc_step": (C.c_int, [vp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "kp_nmpc_step_batch": (C.c_int, [vp, C.c_int, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip]),
    "kp_nmpc_simulate": (C.c_int, [vp, C.c_int, C.c_int, c_dp, C.c_int, c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_ip, c_ip]),
    "kp_nmpc_last_jacobians": (C.c_int, [vp, c_dp]),
    "kp_nmpc_destroy": (C.c_int, [vp]),
}
TIMER_NMPC_SIM = 21                # kp_timer_get slot: the kernel of the most recent kp_nmpc_simulate, ms

# the batched load observer (include/koopman_hip_observer.h)
OBSERVER_SIGNATURES = {
    "kp_load_observe": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp, C.c_int, C.c_int64, c_dp, c_dp, C.c_int,
                                  C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.c_int, c_dp,
                                  C.c_int, c_dp, c_dp, c_ip]),
}
OBS_RATE, OBS_PIN_LAST = 1, 2      # flags of kp_load_observe

# continuous-time models: matrix logarithm and ode45 rollouts (include/koopman_hip_ct.h)
CT_SIGNATURES = {
    "kp_logm": (C.c_int, [vp, C.c_int, C.c_int, c_dp, C.c_double, C.c_double, c_dp, c_ip, c_ip]),
    "kp_rollout_ct": (C.c_int, [vp, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, C.c_double,
                                C.c_double, C.c_double, c_dp, c_ip, c_ip, c_ip]),
    "kp_rollout_nl_ct": (C.c_int, [vp, vp, C.c_int, c_dp, c_dp, c_dp, C.c_int, C.c_double, C.c_double, C.c_double, c_dp, c_ip, c_ip,
                                   c_ip]),
}

# the arm plant (include/koopman_hip_arm.h)
class KpArmParams(C.Structure):
    _fields_ = [("Nmods", C.c_int), ("nlinks", C.c_int), ("l", C.c_double), ("k", C.c_double), ("d", C.c_double),
                ("m", C.c_double), ("i", C.c_double), ("g", C.c_double), ("ku", C.c_double)]


ARM_SIGNATURES = {
    "kp_arm_simulate": (C.c_int, [vp, C.POINTER(KpArmParams), C.c_int, C.c_int, C.c_int, c_dp, C.c_double, c_dp, c_dp, c_dp,
                                  C.c_double, C.c_double, c_dp, c_ip, c_ip, c_ip]),
}
ARM_MODE = {"zoh": 0, "interp": 1, "floor": 2, "restart": 3}      # KP_ARM_SPAN_ZOH, _SPAN_INTERP, _SPAN_FLOOR, KP_ARM_RESTART

# the random-system generator (include/koopman_hip_rsys.h)
class KpRsysDims(C.Structure):
    _fields_ = [("num_terms", C.c_int), ("degree_x", C.c_int), ("degree_u", C.c_int)]


RSYS_SIGNATURES = {
    "kp_rsys_simulate": (C.c_int, [vp, C.POINTER(KpRsysDims), C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, c_ip, c_ip, c_dp,
                                   c_dp, c_dp, C.c_int, C.c_double, C.c_double, c_dp, c_ip, c_ip, c_ip, C.POINTER(vp)]),
}
RSYS_MODE = {"span": 0, "restart": 1}      # KP_RSYS_SPAN, KP_RSYS_RESTART

# the validation table (include/koopman_hip_validate.h)
VALIDATE_SIGNATURES = {
    "kp_validate": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, C.c_int,
                              C.POINTER(C.c_int64), c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int, c_dp, c_ip, c_dp]),
    "kp_validate_ct": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, C.c_int,
                                 C.POINTER(C.c_int64), c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int, C.c_double, C.c_double, C.c_double,
                                 c_dp, c_ip, c_dp, c_ip, c_ip]),
}
# prediction-horizon validation (include/koopman_hip_horizon.h)
HORIZON_SIGNATURES = {
    "kp_validate_horizon": (C.c_int, [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_dp, c_dp, C.c_int,
                                      C.POINTER(C.c_int64), c_dp, c_dp, c_dp, C.c_int, C.c_int, c_dp, C.POINTER(C.c_int64), c_ip]),
}
TIMER_HORIZON = 24                 # kp_timer_get slot: the two kernels of the most recent kp_validate_horizon, ms
TIMER_HORIZON_TILE = 25            # ... and 1000 x (model rows staged in LDS) + the tile width S_T it ran (64, 32 or 16)
TIMER_GRAM3_EARLY_BARRIER = 26     # where the tiles of the last Kronecker Gram launch had their barrier: 1 in front of the last quad steps, 0 behind the last
HORIZON_CHUNK = 8                 # KP_HORIZON_CHUNK
VALIDATE_CHUNK = 128               # KP_VALIDATE_CHUNK
VALIDATE_CT_CHUNK = 32             # KP_VALIDATE_CT_CHUNK
VALIDATE_CT_STAGE = 8192           # KP_VALIDATE_CT_STAGE

# whole closed loops with the model as the plant (include/koopman_hip_sim.h)
SIM_SIGNATURES = {
    "kp_mpc_simulate": (C.c_int, [vp, vp, C.c_int, C.c_int, c_dp, C.c_int, c_dp, c_dp, C.c_int, c_dp, c_dp, c_dp, c_ip, c_ip]),
}
TIMER_MPC_SIM = 19                 # kp_timer_get slot: the kernel of the most recent kp_mpc_simulate, ms

# the Koopman spectrum: batched eigenvalues and eigenvectors of general matrices (include/koopman_hip_spectrum.h)
SPECTRUM_SIGNATURES = {
    "kp_eig": (C.c_int, [vp, C.c_int, C.c_int, c_dp, C.c_int, c_dp, c_dp, c_dp, c_ip, c_ip]),
}
TIMER_EIG = 22                     # kp_timer_get slot: the kernel of the most recent kp_eig, ms
TIMER_EIG_REGIME = 23              # ... and the regime it ran (1 wave per matrix, 2 workgroup in LDS, 3 workgroup in a workspace slot)
EIG_MAXN = 512                     # KP_EIG_MAXN
EIG_WAVE_MAX = 32                  # KP_EIG_WAVE_MAX
EIG_LDS_MAXN_VEC, EIG_LDS_MAXN_VAL = 99, 140      # KP_EIG_LDS_MAXN_VEC, KP_EIG_LDS_MAXN_VAL

# what the lasso fit ran, and its product kernels alone (include/koopman_hip_lasso.h)
LASSO_SIGNATURES = {
    "kp_symm_product": (C.c_int, [vp, c_dp, c_dp, C.c_int, C.c_int, C.c_int, c_dp, c_ip]),
}
TIMER_LASSO_KERNELS = 27           # kp_timer_get slot: bit mask of the kernels the most recent lasso batch's iteration loop launched
LASSO_RAN_EPT = {4: 0x1, 8: 0x2, 16: 0x4, 24: 0x8, 0: 0x10}      # KP_LASSO_RAN_EPT4 ... _EPT0: kp_lasso_project_kernel<EPT>
LASSO_RAN_MULTI = 0x20             # KP_LASSO_RAN_MULTI: the multi-launch projection
LASSO_RAN_SMALL, LASSO_RAN_TILED, LASSO_RAN_NAIVE = 0x40, 0x80, 0x100      # the product kernels
LASSO_RAN_RA = {4: 0x200, 5: 0x400, 6: 0x800, 7: 0x1000, 8: 0x2000}       # KP_LASSO_RAN_RA4 << (RA - 4)
LASSO_RAN_RB = {2: 0x4000, 3: 0x8000, 4: 0x10000, 6: 0x20000}             # KP_LASSO_RAN_RB2 ... _RB6
SYMM_BY_SHAPE, SYMM_SMALL, SYMM_TILED_RB = 0, 1, 10                       # `variant` of kp_symm_product
SYMM_RAN_SMALL, SYMM_RAN_NAIVE, SYMM_RAN_TILED = 1, 2, 1000               # its `ran`: tiled = 1000 + 10 RA + RB

# the TN product of the wide path alone (include/koopman_hip_tn.h)
TN_SIGNATURES = {
    "kp_tn_product": (C.c_int, [vp, c_dp, C.c_int64, c_dp, C.c_int64, C.c_int, C.c_int, C.c_int, c_dp, C.c_int64, C.c_double, C.c_double,
                                C.c_int, C.c_int, c_dp, c_dp, C.c_int, C.c_int, c_ip]),
}
TN_MISALIGN, TN_SAME, TN_MIRROR = 0x1, 0x2, 0x4                           # `flags` of kp_tn_product
TN_RAN_FORM, TN_RAN_VEC = 1000, 100                                       # its `ran`: 1000 form + 100 vec + splits
TN_FORM_SMALL = 4                                                         # the 64 x 64 form (M <= 64)
TN_SHAPES = ((128, 64), (128, 96), (256, 96), (192, 128))                 # `form` 0 ... 3: tng_shapes() of csrc/kp_tn_gemm.h

_lib = None


def lib():
    """Loads libkoopman_hip.so (once).  Raises OSError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OSError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(make -C koopman-realizations_amd/csrc)")
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in (SIGNATURES | NMPC_SIGNATURES | OBSERVER_SIGNATURES | CT_SIGNATURES | ARM_SIGNATURES
                                   | RSYS_SIGNATURES | VALIDATE_SIGNATURES | HORIZON_SIGNATURES | SIM_SIGNATURES | SPECTRUM_SIGNATURES | LASSO_SIGNATURES
                                   | TN_SIGNATURES).items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


class KoopmanHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkoopman_hip error {code}: {msg}")
        self.code = code


def check(rc, ctx=None):
    if rc != KP_OK:
        msg = lib().kp_last_error(ctx)
        raise KoopmanHipError(rc, msg.decode() if msg else "")


def fcol(a, dtype=np.float64):
    """Column-major (MATLAB layout) contiguous f64 copy/view."""
    return np.asfortranarray(np.asarray(a, dtype=dtype))


def dptr(a):
    return None if a is None else a.ctypes.data_as(c_dp)
