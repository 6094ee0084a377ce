"""The random-system generator on the device: `DeviceRsys` is `Rsys` (rsys.py) with every simulation in kp_rsys_simulate
(include/koopman_hip_rsys.h, one GPU lane per (system, trial)).

  * simulate_systems          Rsys.simulate_systems as the reference integrates (Rsys.m:118): ONE ode45 over the time
                              vector per trial, input rows by get_u, outputs from ode45's interpolant
  * simulate_systems_restart  rsys.py's host mirror (simulate_systems / simulate_systems_fast): ode45 restarted at every
                              sample under the held input
  * simulate_to_traj          either of the two straight into a device-resident Traj in the layout of Rsys.save_data, for
                              sweep.rand_models_sweep_traj: generation, scaling, fits and validation without the data
                              crossing to the host
For the same seed the systems and the input levels are Rsys's: the same draws in the same order.
"""
from __future__ import annotations

import numpy as np

from . import _ffi as F
from .rsys import Rsys

HOLD = 50          # samples per input level (Rsys.m:116)


class DeviceRsys(Rsys):
    """Rsys(num_sys, num_terms, degree_x, degree_u, seed) whose simulations run on the device (ctx: a kra.Context,
    default the package's)."""

    def __init__(self, num_sys, num_terms, degree_x, degree_u, seed=0, ctx=None):
        super().__init__(num_sys, num_terms, degree_x, degree_u, seed=seed)
        self._ctx = ctx

    @property
    def ctx(self):
        if self._ctx is None:
            from .ksysid import default_context
            self._ctx = default_context()
        return self._ctx

    def _system_arrays(self):
        co = np.stack([s["coeffs"] for s in self.systems])
        px = np.stack([s["pow_x"] for s in self.systems])
        pu = np.stack([s["pow_u"] for s in self.systems])
        cu = np.array([s["input_gain"] for s in self.systems], dtype=np.float64)
        return co, px, pu, cu

    def _prepare(self, t_end, Ts, num_trials, x0):
        """tq as rsys.py builds it, the trials' initial states, and the input levels of every (system, trial) drawn as
        generate_input_steps draws them (system-major, trial-minor: the order of Rsys.simulate_systems)."""
        x0 = np.atleast_2d(np.asarray(x0, dtype=np.float64))
        if x0.shape[0] == 1:
            x0 = np.repeat(x0, num_trials, axis=0)                       # Rsys.m:104-106
        if x0.shape != (num_trials, 1):
            raise ValueError("DeviceRsys: x0 must be (1, 1) or (num_trials, 1)")
        tq = np.arange(0.0, t_end + 0.5 * Ts, Ts)
        nlev = len(np.arange(0, len(tq), HOLD))
        levels = 2.0 * self.rng.random((self.num_sys, num_trials, nlev)) - 1.0
        return tq, x0[:, 0], levels

    @staticmethod
    def expand_levels(levels, T, hold=HOLD):
        """The input rows of levels (..., nlev) held `hold` samples each, with generate_input_steps' zero tail."""
        levels = np.asarray(levels, dtype=np.float64)
        nlev = levels.shape[-1]
        r = np.arange(T)
        return np.ascontiguousarray(np.where(r < hold * (nlev - 1), levels[..., np.minimum(r // hold, nlev - 1)], 0.0))

    def _simulate(self, mode, t_end, Ts, num_trials, x0, want_traj=False, want_Y=True):
        tq, x0v, levels = self._prepare(t_end, Ts, num_trials, x0)
        co, px, pu, cu = self._system_arrays()
        res = self.ctx.rsys_simulate(mode, tq, co, px, pu, cu, x0v, levels, hold=HOLD, degree_x=self.degree_x,
                                     degree_u=self.degree_u, want_traj=want_traj, want_Y=want_Y)
        Y, na, nr, st = res[:4]
        self.last_stats = {"naccept": na, "nreject": nr, "status": st}
        self.last_Y = Y
        self.last_t = tq
        self._last_levels = levels
        return res

    @property
    def last_U(self):
        """The input rows of the most recent simulation (num_sys, num_trials, len(tq)), expanded from its levels."""
        return self.expand_levels(self._last_levels, len(self.last_t))

    def _check_status(self, st, what):
        bad = np.argwhere(st != F.KP_OK)
        if bad.size:
            raise RuntimeError(f"{what}: ode45 failed (step size underflow, step limit or non-finite state) in "
                               f"(system, trial) {[tuple(b) for b in bad[:8].tolist()]}")

    def _as_data(self, num_trials):
        tq, Y, U = self.last_t, self.last_Y, self.last_U
        return [[{"t": tq.copy(), "y": Y[i, j][:, None].copy(), "u": U[i, j][:, None].copy()} for i in range(self.num_sys)]
                for j in range(num_trials)]

    def simulate_systems(self, t_end, Ts, num_trials, x0):
        """Rsys.m:96-125 as the reference integrates: one ode45 over tq per trial.  Returns data[j][i] = {t, y, u}."""
        st = self._simulate("span", t_end, Ts, num_trials, x0)[3]
        self._check_status(st, "DeviceRsys.simulate_systems")
        return self._as_data(num_trials)

    def simulate_systems_restart(self, t_end, Ts, num_trials, x0):
        """rsys.py's simulate_systems / simulate_systems_fast: ode45 from sample to sample under the held input."""
        st = self._simulate("restart", t_end, Ts, num_trials, x0)[3]
        self._check_status(st, "DeviceRsys.simulate_systems_restart")
        return self._as_data(num_trials)

    def simulate_to_traj(self, t_end, Ts, num_trials, x0, mode="span", keep_host=False):
        """The trials straight into a finished device-resident Traj (Rsys.save_data's layout: trials 0 .. num_trials-2
        train, the last validates; scaling computed on the device), for sweep.rand_models_sweep_traj.  mode: 'span' (the
        reference) or 'restart'.  The trajectories do not come back to the host unless keep_host=True, which also leaves
        the raw outputs in last_Y (num_sys, num_trials, len(tq)); last_U holds the inputs either way."""
        if mode not in F.RSYS_MODE:
            raise ValueError(f"DeviceRsys.simulate_to_traj: mode must be one of {sorted(F.RSYS_MODE)}")
        res = self._simulate(mode, t_end, Ts, num_trials, x0, want_traj=True, want_Y=keep_host)
        self._check_status(res[3], "DeviceRsys.simulate_to_traj")
        return res[4]
