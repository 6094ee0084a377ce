"""The arm plant on the device: `DeviceArm` is `Arm` (arm.py) with every simulation in kp_arm_simulate
(include/koopman_hip_arm.h, one GPU lane per trial).

  * simulate_Ts / simulate / simulate_Ts_batch  arm.py's host conventions (one ode45 restart per sample, Arm.m:932-957),
                                                so Ksim(DeviceArm(...), kmpc) runs the same closed loop as Ksim(Arm(...), ...)
  * simulate_ode45                              Arm.simulate (Arm.m:960-1049): ONE ode45 over the time vector, outputs
                                                from its interpolant, input_type 'zoh' or 'interp'
  * get_rampNhold / simulate_rampNhold          Arm.m:1054-1083 and 866-930 (random ramp-and-hold training trials)
The equations of motion, the output map and the parameters are Arm's.
"""
from __future__ import annotations

import numpy as np

from . import _ffi as F
from .arm import Arm


def _colon(a, d, b):
    """MATLAB's (a : d : b)': the first half of the elements counted from a, the second half back from b."""
    n = int(np.floor((b - a) / d + 1e-10)) + 1
    if n < 1:
        return np.zeros(0)
    last = a + (n - 1) * d
    if abs(last - b) <= 1e-10 * max(abs(a), abs(b), abs(d)):
        last = b
    k = np.arange(n)
    return np.where(k < n // 2, a + k * d, last - (n - 1 - k) * d)


class DeviceArm(Arm):
    """Arm(params, output_type) whose simulations run on the device (ctx: a kra.Context, default the package's)."""

    def __init__(self, params, output_type="angles", ctx=None):
        super().__init__(params, output_type)
        n = int(self.params["Nlinks"])
        if int(self.params["Nmods"]) * int(self.params["nlinks"]) != n:
            raise ValueError("params.Nlinks must equal Nmods * nlinks")
        self._ctx = ctx

    @property
    def ctx(self):
        if self._ctx is None:
            from .ksysid import default_context
            self._ctx = default_context()
        return self._ctx

    # ---- output map, vectorised over rows (the same arithmetic as Arm.get_y row by row) -------------------------
    def get_y(self, x):
        x = np.asarray(x, dtype=np.float64)
        single = x.ndim == 1
        X = np.atleast_2d(x)
        n = int(self.params["Nlinks"])
        if X.shape[1] != 2 * n:
            raise ValueError(f"Input state matrix has wrong dimension. Its width should be {2 * n}")
        if self.output_type == "angles":
            Y = X[:, :n].copy()
        elif self.output_type in ("markers", "endeff"):
            th = np.cumsum(X[:, :n], axis=1)
            J = np.cumsum(self.params["l"] * np.stack([-np.sin(th), np.cos(th)], axis=2), axis=1)    # joints 1..n
            if self.output_type == "markers":
                Y = J[:, int(self.params["nlinks"]) - 1::int(self.params["nlinks"])].reshape(X.shape[0], -1)
            else:
                Y = J[:, -1].copy()
        else:
            raise ValueError(f"output_type {self.output_type!r} is not supported")
        return Y[0] if single else Y

    # ---- one-period steps (RESTART mode) -------------------------------------------------------------------------
    def _run(self, mode, t, U, W, x0=None, Ts=0.0):
        X, na, nr, st = self.ctx.arm_simulate(self.params, mode, t, U, W, x0, Ts)
        self.last_stats = {"naccept": na, "nreject": nr, "status": st}
        return X, st

    def _check_status(self, st, what):
        bad = np.flatnonzero(st != F.KP_OK)
        if bad.size:
            raise RuntimeError(f"{what}: ode45 failed (step size underflow, step limit or non-finite state) in trial(s) {bad.tolist()}")

    def _load(self, w):
        if w is None or np.size(w) == 0:
            return np.zeros(2)
        w = np.asarray(w, dtype=np.float64).ravel()
        if w.size != 2:
            raise ValueError("w must have width of 2")
        return w

    def simulate_Ts_batch(self, X, U, W=None, tstep=None):
        """The state one sampling period later for every row of X (batch x 2 Nlinks) under the held inputs U
        (batch x Nmods) and loads W (batch x 2, or None): simulate_Ts for all rows in one launch."""
        n, nm = int(self.params["Nlinks"]), int(self.params["Nmods"])
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        U = np.atleast_2d(np.asarray(U, dtype=np.float64))
        if X.shape[1] != 2 * n or U.shape != (X.shape[0], nm):
            raise ValueError(f"X must be (batch, {2 * n}) and U (batch, {nm})")
        b = X.shape[0]
        T = self.params["Ts"] if tstep is None else tstep
        Uk = np.repeat(U[:, None, :], 2, axis=1)
        Wk = None
        if W is not None:
            W = np.atleast_2d(np.asarray(W, dtype=np.float64))
            if W.shape[1] != 2:
                raise ValueError("w must have width of 2")
            Wk = np.repeat(np.broadcast_to(W, (b, 2))[:, None, :], 2, axis=1)
        Xo, st = self._run("restart", np.array([0.0, float(T)]), Uk, Wk, X)
        self._check_status(st, "simulate_Ts_batch")
        return Xo[:, 1]

    def simulate_Ts(self, x_k, u_k, w_k=None, tstep=None):
        """Arm.m:932-957 on the device: the state one sampling period later under a held input."""
        w = self._load(w_k)
        return self.simulate_Ts_batch(np.ravel(x_k)[None], np.ravel(u_k)[None], w[None], tstep)[0]

    def simulate(self, t_in, u_in, w_in=None):
        """Arm.simulate as arm.py restates it (one ode45 restart per sample, rest initial condition), in one launch."""
        t_in = np.asarray(t_in, dtype=np.float64).ravel()
        u_in = np.atleast_2d(np.asarray(u_in, dtype=np.float64))
        n = int(self.params["Nlinks"])
        if u_in.shape[0] != t_in.size:
            raise ValueError("t_in and u_in vectors need to be the same length")
        if u_in.shape[1] != int(self.params["Nmods"]):
            raise ValueError("u_in width must be the same as the number of modules")
        w_in = np.zeros((t_in.size, 2)) if w_in is None else np.broadcast_to(np.atleast_2d(w_in), (t_in.size, 2))
        X, st = self._run("restart", t_in - t_in[0], u_in[None], np.asarray(w_in)[None])
        self._check_status(st, "simulate")
        X = X[0]
        return {"t": t_in, "x": X, "alpha": X[:, :n], "alphadot": X[:, n:], "y": self.get_y(X), "u": u_in,
                "w": np.array(w_in), "params": self.params}

    # ---- whole trials (one ode45 over the time vector) -----------------------------------------------------------
    def _trials(self, U, T):
        nm = int(self.params["Nmods"])
        if isinstance(U, (list, tuple)):
            U = [np.atleast_2d(np.asarray(u, dtype=np.float64)) for u in U]
            single = False
        else:
            U = np.asarray(U, dtype=np.float64)
            single = U.ndim <= 2
            U = [np.atleast_2d(U)] if single else list(U)
        for u in U:
            if u.shape[0] != T:
                raise ValueError("t_in and u_in vectors need to be the same length")
            if u.shape[1] != nm:
                raise ValueError("u_in width must be the same as the number of modules")
        return np.stack(U), single

    def _loads(self, W, b, T):
        if W is None:
            return np.zeros((b, T, 2))
        if isinstance(W, (list, tuple)) and len(W) == b and np.ndim(W[0]) >= 1 and np.size(W[0]) != 1:
            return np.stack([self._load_rows(w, T) for w in W])
        W = np.asarray(W, dtype=np.float64)
        if W.ndim == 3:
            if W.shape[0] != b:
                raise ValueError("W must hold one load array per trial")
            return np.stack([self._load_rows(w, T) for w in W])
        return np.broadcast_to(self._load_rows(W, T), (b, T, 2)).copy()

    @staticmethod
    def _load_rows(w, T):
        """Arm.m:971-977: one row stacked over time, or T rows of width 2."""
        w = np.atleast_2d(np.asarray(w, dtype=np.float64))
        if w.shape[0] == 1 and w.shape[1] == 2:
            return np.repeat(w, T, axis=0)
        if w.shape[1] != 2:
            raise ValueError("w_in must have width of 2")
        if w.shape[0] != T:
            raise ValueError("w_in must have one row or as many rows as t_in")
        return w

    def _sims(self, t, X, U, W):
        n = int(self.params["Nlinks"])
        Y = self.get_y(X.reshape(-1, 2 * n)).reshape(X.shape[0], X.shape[1], -1)
        tc = np.asarray(t, dtype=np.float64).reshape(-1, 1)
        return [{"t": tc, "x": X[b], "alpha": X[b, :, :n], "alphadot": X[b, :, n:], "y": Y[b], "u": U[b], "w": W[b],
                 "params": self.params} for b in range(X.shape[0])]

    def simulate_ode45(self, t, U, W=None, input_type="zoh"):
        """Arm.simulate(t_in, u_in, w_in, 'input_type', ...) (Arm.m:960-1049): rest initial condition, ONE ode45 over t
        ('zoh') or t[:-1] ('interp') with outputs from its interpolant; the input / load row of every stage by get_k
        (rules in include/koopman_hip_arm.h).  U: one trial (T x Nmods), a list of them or a (batch, T, Nmods) stack,
        all on the same t; W: None, one load row, T x 2 rows, or one of these per trial.  All trials run in one
        launch.  Returns one sim dict (t, x, alpha, alphadot, y, u, w, params, as Arm.m:1026-1033) per trial, or one
        dict for a single trial; they are usable as Ksysid train / val entries (with w for loaded=True)."""
        if input_type not in ("zoh", "interp"):
            raise ValueError("input_type argument is not valid. Choices are <zoh> or <interp>.")
        t = np.asarray(t, dtype=np.float64)
        if t.ndim == 2 and t.shape[1] != 1:
            raise ValueError("t_in must be a column vector")
        t = t.ravel()
        U, single = self._trials(U, t.size)
        W = self._loads(W, U.shape[0], t.size)
        X, st = self._run(input_type, t - t[0], U, W)
        self._check_status(st, "simulate_ode45")
        Tout = X.shape[1]
        sims = self._sims(t[:Tout], X, U[:, :Tout], W)
        return sims[0] if single else sims

    def get_rampNhold(self, tf, Tramp, lb, ub, rng=None):
        """Arm.m:1054-1083: a random ramp-and-hold signal between lb and ub on tsteps = (0 : Ts : tf)'.  Returns
        (signal, tsteps).  The random table comes from the numpy Generator `rng` (default: a fresh
        np.random.default_rng()), not from MATLAB's stream, so the same seed does not give MATLAB's signal."""
        rng = np.random.default_rng() if rng is None else rng
        lb = np.atleast_1d(np.asarray(lb, dtype=np.float64)); ub = np.atleast_1d(np.asarray(ub, dtype=np.float64))
        if lb.shape != ub.shape or lb.ndim != 1:
            raise ValueError("lb and ub must be vectors of the same length")
        tsteps = _colon(0.0, float(self.params["Ts"]), float(tf))
        tswitch = _colon(0.0, float(Tramp), float(tf))
        nper = int(np.ceil(tswitch.size / 2))
        nohold = (ub - lb) * rng.random((nper, lb.size)) + lb
        hold = np.repeat(nohold, 2, axis=0)[:tswitch.size]
        sig = np.stack([np.interp(tsteps, tswitch, hold[:, j], left=0.0, right=0.0) for j in range(lb.size)], axis=1)
        return sig, tsteps

    def simulate_rampNhold(self, tf, Tramp, w, trials=1, rng=None):
        """Arm.simulate_rampNhold (Arm.m:866-930): `trials` rest-start trials under random ramp-and-hold inputs of
        amplitude params.umax (switch period Tramp, duration tf), each with the constant load w = [end-effector mass,
        gravity angle] (or row b of a (trials, 2) w: a batch of loads, which the reference simulates one call each), in
        one launch.  The input row of every stage is u(floor(t / Ts) + 1, :) as in the reference.
        The inputs are drawn from the numpy Generator `rng` (see get_rampNhold), trial after trial.  Returns one sim
        dict per trial (a list, or one dict for trials=1)."""
        if int(trials) < 1:
            raise ValueError("trials must be at least 1")
        w = np.atleast_2d(np.asarray(w, dtype=np.float64))
        if w.shape[1] != 2 or w.shape[0] not in (1, int(trials)):
            raise ValueError("w must have width of 2 (one row, or one row per trial)")
        if not (float(Tramp) > 0 and float(tf) > 0):
            raise ValueError("tf and Tramp must be positive")
        rng = np.random.default_rng() if rng is None else rng
        umax = float(self.params["umax"])
        nm = int(self.params["Nmods"])
        sigs = [self.get_rampNhold(tf, Tramp, -umax * np.ones(nm), umax * np.ones(nm), rng) for _ in range(int(trials))]
        t = sigs[0][1]
        if t.size < 2:
            raise ValueError("tf must span at least one sampling period")
        U = np.stack([s for s, _ in sigs])
        W = np.broadcast_to(w[:, None, :], (U.shape[0], t.size, 2)).copy()
        X, st = self._run("floor", t, U, W, Ts=float(self.params["Ts"]))
        self._check_status(st, "simulate_rampNhold")
        sims = self._sims(t, X, U, W)
        return sims[0] if int(trials) == 1 else sims
