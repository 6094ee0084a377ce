"""Host-side mirrors of the reference's `Kmpc` (Kmpc.m) and `Ksim` (Ksim.m) classes.

Kmpc keeps the reference's constructor options and method signatures for the QP-based
controllers (model_type 'linear' and 'bilinear' with mpc_type 'linear'); the per-step work —
lift, QP assembly and QP solve — is one kernel launch in libkoopman_hip.so.
Loaded models (sysid_class.loaded): the lifted state is the loaded lift with the current load estimate
traj['what'] (Kmpc.m:347-348, :771-772, :839-840); estimate_load_linear / estimate_load_bilinear (Kmpc.m:1298-1445)
assemble the regression on the host and solve the constrained least squares with the library's QP kernel.
get_mpcInput_loaded does the estimate, the loaded lift and the step in one launch (kp_mpc_step_loaded); a loaded Ksim
uses it when fused_load_step is true (the default) and the host-assembled estimate + step otherwise.
state_bounds (Kmpc.m:300-318) are scaled down like the reference does and handed to kp_mpc_set_state_bounds.
Nonlinear models (model_type 'nonlinear', mpc_type 'nonlinear'): get_mpcInput_nonlinear (Kmpc.m:1114-1181) solves the
reference's fmincon SQP problem by a single-shooting SQP in one kernel launch (kp_nmpc_step), in the one configuration the
reference runs: unloaded, nd = 0; run_simulation is the host loop of such steps with the model as the plant,
run_simulations runs every trial's whole loop in one launch (kp_nmpc_simulate).  Out of scope: bilinear models with mpc_type 'nonlinear', the unused nlmpc glue.
"""
from __future__ import annotations

import time

import numpy as np

from . import _ffi as F
from .device import Mpc, Nmpc


class Kmpc:
    """Model predictive controller (mirror of classdef Kmpc, Kmpc.m:1)."""

    def __init__(self, sysid_class, **kwargs):
        s = sysid_class
        if getattr(s, "time_type", "discrete") == "continuous":     # Kmpc.m never reads time_type: it would build a wrong controller
            raise ValueError("Kmpc needs a discrete-time model: this Ksysid has time_type='continuous'")
        self.sysid = s
        self.ctx = s.ctx
        self.params = s.params                      # Kmpc.m:44
        self.model = s.model
        self.lift = s.lift
        self.basis = s.basis
        self.model_type = s.model_type              # :51
        self.loaded = s.loaded
        # defaults (:55-72)
        self.horizon = int(np.floor(1.0 / self.params["Ts"]))
        self.input_bounds = None
        self.input_slopeConst = None
        self.input_smoothConst = None
        self.state_bounds = None
        self.cost_running = 0.1
        self.cost_terminal = 100.0
        self.cost_input = 0.0
        self.projmtx = self.model["C"]
        self.load_obs_horizon = 10                  # :66-67 (loaded models: past samples of the load observer's window)
        self.load_obs_period = 1                    # (steps between load estimates)
        self.fused_load_step = True                 # Ksim: estimate + lift + step in one launch (get_mpcInput_loaded)
        self.nmpc_max_iter = 60                     # nonlinear MPC: SQP iteration cap of one step (measured counts)
        self.nmpc_tol = 1e-8                        #   tolerance of its stopping test (KKT residual and step)
        self.nmpc_damping = 10.0                    #   initial Levenberg-Marquardt damping of its QP Hessian
        self.nmpc_warm_start = False                #   start from the shifted previous solution instead of the reference's X0
        self.mpc_type = "nonlinear" if self.model_type == "nonlinear" else "linear"
        for k, v in kwargs.items():                 # parse_args :107-113
            if not hasattr(self, k):
                raise AttributeError(f"unknown Kmpc property {k}")
            setattr(self, k, v)
        if isinstance(self.input_bounds, (list, tuple, np.ndarray)) and np.size(self.input_bounds) == 0:
            self.input_bounds = None
        if isinstance(self.state_bounds, (list, tuple, np.ndarray)) and np.size(self.state_bounds) == 0:
            self.state_bounds = None
        if self.mpc_type == "nonlinear" and self.model_type != "nonlinear":
            raise NotImplementedError(f"mpc_type 'nonlinear' with a {self.model_type} model: the reference's get_BLmodel defines no "
                                      "F_sym (Ksysid.m:1248-1278), which get_constraintMatrices_nonlinear needs (Kmpc.m:1054-1057)")
        if self.model_type == "nonlinear":
            if self.mpc_type != "nonlinear":
                raise NotImplementedError("a nonlinear model has no linear MPC: get_costMatrices needs the model's A and B "
                                          "(Kmpc.m:160-200), get_NLmodel defines only F (Ksysid.m:1298-1341)")
            if self.loaded:
                raise NotImplementedError("nonlinear MPC of a loaded model: nonlcon_nmpc calls F_func(z, u) with two arguments "
                                          "(Kmpc.m:1091), the loaded model's F takes the load as a third")
            if int(self.params.get("nd", 0)) > 0:
                raise NotImplementedError("nonlinear MPC with delays (nd > 0): nonlcon_nmpc indexes the states by n "
                                          "(Kmpc.m:1087-1091) while F returns nzeta = n (nd + 1) entries")
        self.projmtx = np.atleast_2d(np.asarray(self.projmtx, dtype=np.float64))
        self.expand_props()                         # :82
        m = self.params["m"]
        sc = self.params["scale"]
        ci = np.asarray(self.cost_input, dtype=np.float64)
        r = np.full(m, float(ci)) if ci.ndim == 0 else ci.reshape(-1)   # eye(m).*cost_input  :201,548
        lo = hi = None
        if self.input_bounds is not None:           # :247,659  scaled-down bounds
            lo = (self.input_bounds[:, 0] - sc["u_offset"]) / sc["u_factor"]
            hi = (self.input_bounds[:, 1] - sc["u_offset"]) / sc["u_factor"]
        slope = None if self.input_slopeConst is None else float(self.input_slopeConst) * float(np.mean(sc["u_factor"]))  # :272,684
        smooth = None if self.input_smoothConst is None else \
            self.params["Ts"] ** 2 * float(self.input_smoothConst) * float(np.mean(sc["u_factor"]))                       # :294,706
        self._U_last = None
        if self.model_type == "nonlinear":                                  # get_cost/constraintMatrices_nonlinear (:909-1059)
            n = self.params["n"]
            self.dev = Nmpc(self.ctx, self.sysid.basis_dev, self.model["Kf"], self.horizon, self.projmtx[:, :n],
                            self.cost_running, self.cost_terminal, r, lo, hi, slope, smooth)
            self.dev.set_options(int(self.nmpc_max_iter), float(self.nmpc_tol), float(self.nmpc_tol), float(self.nmpc_damping))
        else:
            self.dev = Mpc(self.ctx, self.model_type, self.model["A"], self.model["B"], self.horizon, self.projmtx,
                           self.cost_running, self.cost_terminal, r, lo, hi, slope, smooth)
        if self.state_bounds is not None:                                   # :313 / :1050 state_bounds_sc = scaledown.y(state_bounds')'
            self.dev.set_state_bounds((self.state_bounds[:, 0] - sc["y_offset"]) / sc["y_factor"],
                                      (self.state_bounds[:, 1] - sc["y_offset"]) / sc["y_factor"])

    # ---- Kmpc.m:116-130 -------------------------------------------------------------------
    def expand_props(self):
        m = self.params["m"]
        if self.input_bounds is not None:
            b = np.atleast_2d(np.asarray(self.input_bounds, dtype=np.float64))
            if b.shape[0] != m:
                b = np.kron(np.ones((m, 1)), b)
            self.input_bounds = b
        if self.state_bounds is not None:                                   # :126-129
            n = self.params["n"]
            sb = np.atleast_2d(np.asarray(self.state_bounds, dtype=np.float64))
            if sb.shape[0] != n:
                sb = np.kron(np.ones((n, 1)), sb)
            self.state_bounds = sb

    # ---- Kmpc.m:135-152 --------------------------------------------------------------------
    def _ref_index(self):
        n = self.params["n"]
        return np.nonzero(self.projmtx[:, :n].sum(axis=0))[0]

    def scaledown_ref(self, ref):
        idx = self._ref_index(); sc = self.params["scale"]
        return (np.atleast_2d(ref) - sc["y_offset"][idx]) / sc["y_factor"][idx]

    def scaleup_ref(self, ref_sc):
        idx = self._ref_index(); sc = self.params["scale"]
        return np.atleast_2d(ref_sc) * sc["y_factor"][idx] + sc["y_offset"][idx]

    # ---- per-step entry points ----------------------------------------------------------------
    def _zeta(self, traj):
        _, zeta = self.sysid.get_zeta(traj)
        return zeta[-1]                                               # Kmpc.m:343-344

    def _pad_ref(self, ref):
        """Kmpc.m:354-365."""
        Np = self.horizon
        ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
        if ref.shape[1] != self.projmtx.shape[0]:
            raise ValueError("Reference trajectory is not the correct dimension")
        if ref.shape[0] > Np + 1:
            ref = ref[:Np + 1]
        elif ref.shape[0] < Np + 1:
            ref = np.vstack([ref, np.tile(ref[-1], (Np + 1 - ref.shape[0], 1))])
        return ref.reshape(-1)

    def _step(self, traj, ref, iters):
        zeta = self._zeta(traj)
        u_prev = np.atleast_2d(traj["u"])[-1]
        if self.loaded:                                                # Kmpc.m:347-348: lift with the load estimate
            z = self.lift.econ_full_loaded(zeta, np.atleast_2d(traj["what"])[-1])
            U, st = self.dev.step(z, u_prev, self._pad_ref(ref), iters)
            return U, z
        U, z, st = self.dev.step_zeta(self.sysid.basis_dev, zeta, u_prev, self._pad_ref(ref), iters)
        return U, z                                                    # U is NaN when the QP failed

    # ---- load estimation (Kmpc.m:1298-1445) ------------------------------------------------------------
    def _lsqlin_load(self, Cl, dl, whatpast, pin_last_zero):
        """The lsqlin call (Kmpc.m:1354, :1442): min ||C x - d||^2, x = [1; w], x_1 = 1, -1 <= w <= 1 and, with a
        previous estimate, |w_i - whatpast_i| <= 0.01.  Strictly convex QP in the free loads, solved by kp_qp_solve."""
        nw = self.params["nw"]
        free = list(range(nw - 1)) if (pin_last_zero and nw >= 1) else list(range(nw))
        what = np.zeros(nw)
        if free:
            Cf = Cl[:, 1:][:, free]
            r = dl - Cl[:, 0]
            rows, rhs = [], []
            for k, i in enumerate(free):
                lo, hi = -1.0, 1.0
                if whatpast is not None:
                    wp = np.atleast_2d(whatpast)[-1]
                    lo, hi = max(lo, wp[i] - 0.01), min(hi, wp[i] + 0.01)
                e = np.zeros(len(free)); e[k] = 1.0
                rows += [e, -e]; rhs += [hi, -lo]
            what[free] = self.ctx.qp_solve(2.0 * Cf.T @ Cf, -2.0 * Cf.T @ r, np.array(rows), np.array(rhs))[0]
        res = Cl @ np.concatenate([[1.0], what]) - dl
        return what, float(res @ res)

    def estimate_load_linear(self, ypast, upast, whatpast=None):
        """Kmpc.m:1298-1356.  The shipped code pins the LAST load to zero through the debugging equality
        Aeq = blkdiag(1, 0, 1) (:1350), which only has the right size for nw = 2; reproduced for nw = 2."""
        p = self.params; N, nz, nw, nd = p["N"], p["nzeta"], p["nw"], p["nd"]
        ypast = np.atleast_2d(ypast); upast = np.atleast_2d(upast)
        if ypast.shape[0] != upast.shape[0]:
            raise ValueError("Input arguments must have the same number of rows")
        _, zp = self.sysid.get_zeta({"y": ypast, "u": upast})
        G = self.lift.econ_full(zp[:-1])                                # psi of every past state, one device call
        CA, CB = self.model["A"][:nz, :], self.model["B"][:nz, :]
        rows = [CA @ np.kron(np.eye(nw + 1), g[:, None]) for g in G]      # :1320-1326
        rhs = [zp[i + 1, :nz] - CB @ upast[nd + i] for i in range(len(G))]
        return self._lsqlin_load(np.vstack(rows), np.concatenate(rhs), whatpast, nw == 2)

    def estimate_load_bilinear(self, ypast, upast, whatpast=None):
        """Kmpc.m:1360-1444."""
        p = self.params; N, nz, nw, m = p["N"], p["nzeta"], p["nw"], p["m"]
        NL = N * (nw + 1)
        ypast = np.atleast_2d(ypast); upast = np.atleast_2d(upast)
        if ypast.shape[0] != upast.shape[0]:
            raise ValueError("Input arguments must have the same number of rows")
        _, zp = self.sysid.get_zeta({"y": ypast, "u": upast})
        G = self.lift.econ_full(zp[:-1])
        A, B = self.model["A"], self.model["B"]
        rows = []
        for i, g in enumerate(G):
            Om = np.kron(np.eye(nw + 1), g[:, None])
            rows.append((A[:nz, :] + sum(upast[i, j] * B[:nz, j * NL:(j + 1) * NL] for j in range(m))) @ Om)   # :1384-1394
        rhs = [zp[i + 1, :nz] for i in range(len(G))]
        return self._lsqlin_load(np.vstack(rows), np.concatenate(rhs), whatpast, False)

    def get_mpcInput_loaded(self, traj, ref, ypast, upast, estimate=True, whatpast=None, iters=1):
        """One step of a loaded controller with the load observer fused in (kp_mpc_step_loaded): with `estimate`, the
        estimate_load_linear / _bilinear of the window (ypast, upast) (Kmpc.m:1298-1444; whatpast adds the rate rows),
        else the lift uses traj['what'] as it is; then the loaded lift and get_mpcInput / get_mpcInput_bilinear_iter(.., iters)
        (Kmpc.m:329-387, :817-904), state bounds included.  Returns (U, z, what) with `what` scaled down; the residual norm of the estimate is
        kept in self.last_resnorm."""
        if not self.loaded:
            raise ValueError("get_mpcInput_loaded needs a loaded model")
        p = self.params; nw, nd, m = p["nw"], p["nd"], p["m"]
        zeta = self._zeta(traj)
        u_prev = np.atleast_2d(traj["u"])[-1]
        flags = 0
        if estimate:
            ypast = np.atleast_2d(ypast); upast = np.atleast_2d(upast)
            if ypast.shape[0] != upast.shape[0]:
                raise ValueError("Input arguments must have the same number of rows")
            _, zwin = self.sysid.get_zeta({"y": ypast, "u": upast})
            nobs = zwin.shape[0] - 1
            # the input of past sample i as the reference indexes it: upast(nd + i) (linear, Kmpc.m:1328-1335), upast(i) (bilinear, :1388-1393)
            uwin = upast[nd:nd + nobs] if self.model_type == "linear" else upast[:nobs]
            wprev = None if whatpast is None else np.atleast_2d(whatpast)[-1]
            if wprev is not None:
                flags |= Mpc.LOAD_RATE
            if self.model_type == "linear" and nw == 2:
                flags |= Mpc.LOAD_PIN_LAST
        else:
            zwin, uwin, wprev = np.zeros((1, p["nzeta"])), np.zeros((0, m)), np.atleast_2d(traj["what"])[-1]
        U, z, what, rn, st = self.dev.step_loaded(self.sysid.basis_dev, nw, zwin, uwin, wprev, flags, zeta, u_prev,
                                                  self._pad_ref(ref), int(iters))
        self.last_resnorm = rn
        return U, z, what

    def get_mpcInput_nonlinear(self, traj, ref):
        """Kmpc.m:1114-1181: one SQP on the device.  Returns (U, z): U (Np x m, row 1 = the pinned u_prev; NaN when a QP
        subproblem failed), z = [zeta; 0] as the reference returns it (:1180).  self.last_info: (SQP iterations, KKT
        residual, status)."""
        if self.model_type != "nonlinear":
            raise ValueError("get_mpcInput_nonlinear needs a nonlinear model")
        zeta = self._zeta(traj)
        u_prev = np.atleast_2d(traj["u"])[-1]
        U_init = None
        if self.nmpc_warm_start and self._U_last is not None and not np.isnan(self._U_last).any():
            U_init = np.vstack([self._U_last[1:], self._U_last[-1:]])    # the previous solution shifted by one step
        U, _, info, st = self.dev.step(zeta, u_prev, self._pad_ref(ref), U_init)
        self._U_last = U
        self.last_info = (int(info[0]), float(info[1]), st)
        z = np.concatenate([zeta, np.zeros(self.params["N"] - len(zeta))])
        return U, z

    def get_mpcInput(self, traj, ref):
        """Kmpc.m:329-387 (linear model)."""
        return self._step(traj, ref, 1)

    def get_mpcInput_bilinear(self, traj, ref):
        """Kmpc.m:750-814."""
        return self._step(traj, ref, 1)

    def get_mpcInput_bilinear_iter(self, traj, ref, iter=1):
        """Kmpc.m:817-904."""
        return self._step(traj, ref, int(iter))

    # ---- Kmpc.m:403-512 ---------------------------------------------------------------------------
    def run_simulation(self, ref_y, y0=None, u0=None):
        """Closed loop with the identified model as the plant (delays = 0).  A nonlinear controller takes one SQP launch per
        step (get_mpcInput_nonlinear) with the plant step F(zeta, u_{k-1}) on the host, and adds nmpc_info: (SQP iterations,
        KKT residual, status) of every step, as Ksim does; its warm start (nmpc_warm_start) begins anew with every run."""
        p = self.params
        n, m = p["n"], p["m"]
        s = self.sysid
        y0 = np.zeros(n) if y0 is None else np.asarray(y0, dtype=np.float64)
        u0 = np.zeros(m) if u0 is None else np.asarray(u0, dtype=np.float64)
        ref_sc = self.scaledown_ref(ref_y)
        res = {"T": [0.0], "U": [u0], "Y": [y0], "K": [0], "R": [np.atleast_2d(ref_y)[0]], "Z": [], "comp_time": []}
        nonlinear = self.model_type == "nonlinear"
        # the controller step (cur, reference window) -> (U, z) and the plant step (cur, z) -> scaled y_k, which sees
        # u_{k-1}: the one-step input delay of Kmpc.m:495
        if nonlinear:
            self._U_last = None
            res["nmpc_info"] = []
            step = self.get_mpcInput_nonlinear
            plant = lambda cur, z: self.model["F_func"](cur["y"][0], cur["u"][0])
        elif self.model_type == "linear":
            step = self.get_mpcInput
            plant = lambda cur, z: self.model["C"] @ (self.model["A"] @ z + self.model["B"] @ cur["u"][0])
        else:
            step = self.get_mpcInput_bilinear
            plant = lambda cur, z: self.model["C"] @ (self.model["A"] @ z + self.model["Beta"](z) @ cur["u"][0])
        k = 1
        while k < ref_sc.shape[0]:
            cur = {"y": s.scaledown_y(res["Y"][-1])[None, :], "u": s.scaledown_u(res["U"][-1])[None, :]}
            t0 = time.perf_counter()
            U, z = step(cur, ref_sc[k - 1:k + self.horizon])
            res["comp_time"].append(time.perf_counter() - t0)
            if nonlinear:
                res["nmpc_info"].append(self.last_info)
            if np.isnan(U).any():
                break
            res["T"].append(k * p["Ts"]); res["U"].append(s.scaleup_u(U[1])); res["Y"].append(s.scaleup_y(plant(cur, z)))
            res["K"].append(k); res["R"].append(self.scaleup_ref(ref_sc[k - 1])[0]); res["Z"].append(z)
            k += 1
        out = {k_: np.array(v) for k_, v in res.items()}
        if nonlinear:
            out["Z"] = out["Z"].reshape(-1, p["N"])
            out["nmpc_info"] = out["nmpc_info"].reshape(-1, 3)
        return out

    # ---- Kmpc.m:390-399 ---------------------------------------------------------------------------
    def resample_ref(self, ref):
        """The reference {t, y} resampled at the model's sampling time: tr = 0 : Ts : t(end), interp1(t, y, tr)."""
        Ts = float(self.params["Ts"])
        t = np.asarray(ref["t"], dtype=np.float64).reshape(-1)
        y = np.asarray(ref["y"], dtype=np.float64)
        y = y.reshape(-1, 1) if y.ndim == 1 else y
        if y.shape[0] != t.size:
            raise ValueError("ref['y'] must have one row per entry of ref['t']")
        tr = np.arange(int(np.floor(t[-1] / Ts + 1e-9)) + 1) * Ts       # the colon's last element does not pass t(end)
        return np.column_stack([np.interp(tr, t, y[:, j]) for j in range(y.shape[1])])

    def run_simulations(self, refs, y0s=None, u0s=None):
        """run_simulation for many trials in ONE launch (kp_mpc_simulate): the whole loop of every trial - lift, step, model
        step - runs on the device, one workgroup per trial.  refs: one reference for every trial, or a list of them (all of
        the same length once sampled at Ts); a reference is an array with a row per sample or a dict {t, y}, which goes
        through resample_ref.  y0s / u0s: (trials, n) / (trials, m) initial outputs and inputs (None: zeros; one row serves
        every trial).  Returns a list with one dict per trial: run_simulation's fields T, U, Y, K, R, Z scaled up, cut
        behind the last completed step, steps_done, and comp_time = the kernel's time divided by the steps it ran, for
        every step.  Models with delays, loaded models and linear / bilinear controllers with state bounds have no device
        loop: they run through run_simulation, trial by trial.  Nonlinear controllers run in one launch too
        (kp_nmpc_simulate, state bounds included) and add nmpc_info per trial."""
        p = self.params
        n, m = p["n"], p["m"]
        s = self.sysid
        one = isinstance(refs, dict) or (not isinstance(refs, (list, tuple)) and np.ndim(refs) <= 2)
        ref_list = [refs] if one else list(refs)
        ref_list = [self.resample_ref(r) if isinstance(r, dict) else np.atleast_2d(np.asarray(r, dtype=np.float64)) for r in ref_list]
        y0s = None if y0s is None else np.atleast_2d(np.asarray(y0s, dtype=np.float64))
        u0s = None if u0s is None else np.atleast_2d(np.asarray(u0s, dtype=np.float64))
        nb = max(len(ref_list), 1 if y0s is None else y0s.shape[0], 1 if u0s is None else u0s.shape[0])
        for name, a in (("refs", ref_list), ("y0s", y0s), ("u0s", u0s)):
            if a is not None and len(a) not in (1, nb):
                raise ValueError(f"{name} has {len(a)} entries for {nb} trials")
        y0s = np.zeros((nb, n)) if y0s is None else np.broadcast_to(y0s, (nb, n))
        u0s = np.zeros((nb, m)) if u0s is None else np.broadcast_to(u0s, (nb, m))
        if self.model_type == "nonlinear":
            return self._run_simulations_nonlinear(ref_list, y0s, u0s)
        if (self.loaded or self.state_bounds is not None or int(p.get("nd", 0)) > 0):
            out = []
            for i in range(nb):
                r = self.run_simulation(ref_list[i if len(ref_list) > 1 else 0], y0s[i], u0s[i])
                r["steps_done"] = len(r["K"]) - 1
                out.append(r)
            return out
        ref_sc = self._stack_refs(ref_list)
        U, Y, Z, sd, st = self.dev.simulate(self.sysid.basis_dev, ref_sc, s.scaledown_y(y0s), s.scaledown_u(u0s), 1, True)
        return self._trial_dicts(ref_list, ref_sc, y0s, u0s, U, Y, sd, F.TIMER_MPC_SIM, lambda i, k: Z[i, :k - 1].copy())

    def _stack_refs(self, ref_list):
        """The scaled-down references of a batched run: (nref, nproj) when one serves every trial, else (nb, nref, nproj)."""
        if any(r.shape != ref_list[0].shape for r in ref_list):
            raise ValueError("run_simulations: every reference must have the same number of rows")
        return self.scaledown_ref(ref_list[0]) if len(ref_list) == 1 else np.stack([self.scaledown_ref(r) for r in ref_list])

    def _trial_dicts(self, ref_list, ref_sc, y0s, u0s, U, Y, sd, timer, Z_of, extra=None):
        """run_simulation's dict for every trial of a batched run, scaled up and cut behind the last completed step.  timer:
        the slot of the launch's kernel time; Z_of(i, k): trial i's Z rows; extra(i, k): fields that go before steps_done."""
        p, s = self.params, self.sysid
        steps = int(sd.sum())
        per_step = self.ctx.timer(timer) * 1e-3 / steps if steps else 0.0
        out = []
        for i in range(len(sd)):
            k = int(sd[i]) + 1                                         # rows 0 .. steps_done
            ref_i = ref_list[i if len(ref_list) > 1 else 0]
            rs = ref_sc if ref_sc.ndim == 2 else ref_sc[i]
            R = np.vstack([ref_i[:1], self.scaleup_ref(rs[:k - 1])]) if k > 1 else ref_i[:1].copy()
            out.append({"T": np.arange(k) * p["Ts"], "U": np.vstack([u0s[i:i + 1], s.scaleup_u(U[i, 1:k])]),
                        "Y": np.vstack([y0s[i:i + 1], s.scaleup_y(Y[i, 1:k])]), "K": np.arange(k), "R": R, "Z": Z_of(i, k),
                        "comp_time": np.full(k - 1, per_step), **(extra(i, k) if extra else {}), "steps_done": int(sd[i])})
        return out

    def _run_simulations_nonlinear(self, ref_list, y0s, u0s):
        """run_simulations for a nonlinear controller: every trial's loop in ONE launch (kp_nmpc_simulate), state bounds
        included; warm = nmpc_warm_start.  Each dict also holds nmpc_info, (SQP iterations, KKT residual, status) per step."""
        s, N, n = self.sysid, self.params["N"], self.params["n"]
        ref_sc = self._stack_refs(ref_list)
        U, Y, info, sd, st = self.dev.simulate(ref_sc, s.scaledown_y(y0s), s.scaledown_u(u0s), bool(self.nmpc_warm_start))

        def Z_of(i, k):                     # [zeta; 0] as get_mpcInput_nonlinear returns it (Kmpc.m:1180)
            Z = np.zeros((k - 1, N))
            Z[:, :n] = Y[i, :k - 1]
            return Z
        return self._trial_dicts(ref_list, ref_sc, y0s, u0s, U, Y, sd, F.TIMER_NMPC_SIM, Z_of,
                                 lambda i, k: {"nmpc_info": info[i, :k - 1].copy()})


class Ksim:
    """Closed-loop simulator (mirror of classdef Ksim, Ksim.m:1).  `system_class` must offer
    simulate_Ts(x, u, w) -> x+ and get_y(x) -> y, like the reference's Arm class, plus
    params['nx'], params['nu']."""

    def __init__(self, system_class, mpc_class):
        self.sys = system_class
        self.mpc = mpc_class

    def _load_rows(self, load_value, nref, check_width):
        """Ksim.m:79-104: the load of every step, or the reference's error for a wrong shape."""
        lv = np.asarray(load_value, dtype=np.float64)
        lv = lv.reshape(1, -1) if lv.ndim <= 1 else lv
        if check_width:
            nw = int(self.sys.params.get("nw", self.mpc.params["nw"]))
            if lv.shape[1] != nw:
                raise ValueError(f"Load argument should have {nw} columns, not {lv.shape[1]}")
            if lv.size == 0:
                return np.zeros((nref, nw))
        if lv.shape[0] == 1:                                                  # constant load
            return np.tile(lv, (nref, 1))
        if lv.shape[0] != nref:
            raise ValueError("Load argument must have 1 or the same number of rows as ref argument")
        return lv

    def run_trial_mpc(self, ref, x0=None, u0=None, load_value=None):
        """Ksim.m:47-262: the closed loop of the controller and the plant over the reference `ref` (rows: samples).
        x0, u0: the initial state and input, held over the nd + 1 rows of the delayed history (:63-76); the controller
        sees the last nd + 1 outputs and inputs (:153-166).  load_value: the true load of the plant, one row (constant)
        or one row per row of ref (:79-104); a loaded model requires it.  Loaded models estimate the load every
        load_obs_period steps over the last load_obs_horizon + 1 samples (:169-194) and lift with the estimate; with
        mpc.fused_load_step the estimate, lift and step are one launch, otherwise the host assembles the estimate.
        The plant steps with the load of the sample the step starts from (results W, row k - 1 in 0-based rows).
        Result fields as in the reference (What: the scaled-up estimates, a zero first row).  comp_time: the reference's
        tic (Ksim.m:205) comes after the load estimate; the host-assembled path times the same span, the fused path's time
        includes the estimate, which runs inside the same launch - the two paths' comp_time measure different work.
        Nonlinear controllers add results['nmpc_info']: (SQP iterations, KKT residual, status) of every step (status
        KP_ERR_NOT_CONVERGED: the step returned its last iterate)."""
        mpc, s = self.mpc, self.mpc.sysid
        Np, nd = mpc.horizon, int(mpc.params["nd"])
        nx, nu = int(self.sys.params["nx"]), int(self.sys.params["nu"])
        ref = np.atleast_2d(np.asarray(ref, dtype=np.float64))
        nref = ref.shape[0]
        x0 = np.zeros((nd + 1, nx)) if x0 is None else np.tile(np.asarray(x0, dtype=np.float64).ravel(), (nd + 1, 1))
        u0 = np.zeros((nd + 1, nu)) if u0 is None else np.tile(np.asarray(u0, dtype=np.float64).ravel(), (nd + 1, 1))
        y0 = np.array([np.asarray(self.sys.get_y(x), dtype=np.float64) for x in x0])
        w = None
        if mpc.loaded:
            if load_value is None:
                raise ValueError("Missing argument: The model expects a load condition but none was provided")
            w = self._load_rows(load_value, nref, True)
        elif load_value is not None:                    # the model has no load, the plant carries one
            w = self._load_rows(load_value, nref, False)
        ref_sc = mpc.scaledown_ref(ref)                                       # Ksim.m:113
        res = {"T": [0.0], "U": [u0[-1]], "Y": [y0[-1]], "K": [0], "R": [ref[0]], "X": [x0[-1]], "Z": [], "comp_time": [],
               "err": []}
        if mpc.loaded:
            res["What"] = [np.zeros(w.shape[1])]                              # :139-144
        proj = mpc.projmtx[:, :mpc.params["n"]]
        Ho, period = int(mpc.load_obs_horizon), int(mpc.load_obs_period)
        k = 1
        while k < ref_sc.shape[0]:                                            # :147
            if k == 1:                                                        # :153-166
                cy, cu = y0, u0
            elif k < nd + 1:
                cy, cu = np.vstack([y0[k - 1:-1], res["Y"]]), np.vstack([u0[k - 1:-1], res["U"]])
            else:
                cy, cu = np.array(res["Y"][-(nd + 1):]), np.array(res["U"][-(nd + 1):])
            cur = {"y": s.scaledown_y(cy), "u": s.scaledown_u(cu)}
            refhor = ref_sc[k - 1:k + Np]                                     # :198-202 (1-based k : k+Np)
            if mpc.loaded:                                                    # :169-194
                if k < nd + 2:                                                # minimum size nd + 2
                    yp, up = np.tile(s.scaledown_y(y0), (nd + 2, 1)), np.tile(s.scaledown_u(u0), (nd + 2, 1))
                elif k < Ho + 1:
                    yp = s.scaledown_y(np.vstack([y0[k - 1:-1], res["Y"]]))
                    up = s.scaledown_u(np.vstack([u0[k - 1:-1], res["U"]]))
                else:
                    yp, up = s.scaledown_y(np.array(res["Y"][-(Ho + 1):])), s.scaledown_u(np.array(res["U"][-(Ho + 1):]))
                estimate = k % period == 0
                if not estimate:
                    cur["what"] = s.scaledown_w(res["What"][-1])
                if mpc.fused_load_step:
                    t0 = time.perf_counter()
                    U, z, what = mpc.get_mpcInput_loaded(cur, refhor, yp, up, estimate=estimate)
                    comp = time.perf_counter() - t0
                    cur["what"] = what
                else:
                    if estimate:
                        est = mpc.estimate_load_linear if mpc.model_type == "linear" else mpc.estimate_load_bilinear
                        cur["what"] = est(yp, up)[0]
                    t0 = time.perf_counter()
                    U, z = mpc._step(cur, refhor, 1)
                    comp = time.perf_counter() - t0
                res["What"].append(s.scaleup_w(cur["what"]))
            else:
                t0 = time.perf_counter()                                      # :205
                if mpc.model_type == "linear":
                    U, z = mpc.get_mpcInput(cur, refhor)
                elif mpc.model_type == "nonlinear":                           # :214-215
                    U, z = mpc.get_mpcInput_nonlinear(cur, refhor)
                    res.setdefault("nmpc_info", []).append(mpc.last_info)     # (iterations, KKT residual, status) of the SQP
                else:
                    U, z = mpc.get_mpcInput_bilinear_iter(cur, refhor, 1)     # :210
                comp = time.perf_counter() - t0
            if np.isnan(U).any():                                             # :220-222
                break
            u_kp1 = s.scaleup_u(U[1])                                         # :225-228
            w_k = None if w is None else w[k - 1]                             # :239-245 results.W(k,:), 1-based k
            x_kp1 = np.asarray(self.sys.simulate_Ts(res["X"][-1], res["U"][-1], w_k), dtype=np.float64)
            y_kp1 = np.asarray(self.sys.get_y(x_kp1), dtype=np.float64)
            res["T"].append(k * mpc.params["Ts"]); res["U"].append(u_kp1); res["Y"].append(y_kp1); res["K"].append(k)
            res["R"].append(mpc.scaleup_ref(ref_sc[k - 1])[0]); res["X"].append(x_kp1); res["Z"].append(z)
            res["comp_time"].append(comp)
            res["err"].append(float(np.sqrt(((res["R"][-1] - proj @ y_kp1) ** 2).sum())))   # :258
            k += 1
        out = {k_: np.array(v) for k_, v in res.items()}
        if w is not None:
            out["W"] = w
        return out


class ModelPlant:
    """Plant adapter that steps the identified Koopman model itself (the role Arm plays in
    example_control.m; the true arm dynamics are out of scope)."""

    def __init__(self, sysid_class):
        self.s = sysid_class
        self.params = {"nx": sysid_class.params["n"], "nu": sysid_class.params["m"]}

    def get_y(self, x):
        return np.asarray(x, dtype=np.float64)

    def simulate_Ts(self, x, u, w=None):
        s = self.s
        z = s.lift.econ_full(s.scaledown_y(x))
        us = s.scaledown_u(u)
        if s.model_type == "linear":
            z1 = s.model["A"] @ z + s.model["B"] @ us
        else:
            z1 = s.model["A"] @ z + s.model["Beta"](z) @ us
        return s.scaleup_y(s.model["C"] @ z1)
