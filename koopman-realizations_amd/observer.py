"""Window planning of the load observer's validation runs (Ksysid.val_observer_load, Ksysid.m:2033-2075, and
val_observer_load_sparse, :2079-2139): pure numpy, no device.

The reference walks a trial of T samples with a history of hor rows that starts as zeros (:2046-2047, :2099-2100) and
shifts one sample in per step i = 1 .. T-1 (newest at the end), estimating the load from the history at step i into
what(i+1).  The history at step i holds zeta(i-hor+1 .. i) and the inputs pushed at steps i-hor+1 .. i, zeros for steps
before 1.  That is window i - 1 (0-based start) of the trial padded in front by hor - 1 zero rows, so every window of a
trial reads one padded array:
  - val_observer_load pushes u(i) (:2048), so row k of the padded inputs is u of the same sample as row k of zeta;
  - val_observer_load_sparse pushes u(i+1) (:2106), a one-step shift the mirror reproduces: the padded inputs are
    u(2 .. T) behind the zeros;
  - the sparse variant estimates only at the steps with mod(i, update_hor) == 0 (:2117).
Zero rows are lifted like any other state (psi(0) is not zero), as the reference's lift of its zero history is.
"""
from __future__ import annotations

import numpy as np


def plan_val_observer(zeta, u, hor, update_hor=None):
    """(zpad, upad, steps) of one trial: the padded rows (hor - 1 + T each) and the steps i (1-based) whose estimates are
    made; the window of step i starts at padded row i - 1.  update_hor None: val_observer_load (every step, u(i));
    else val_observer_load_sparse (steps with i % update_hor == 0, u(i+1))."""
    zeta = np.atleast_2d(np.asarray(zeta, dtype=np.float64))
    T = zeta.shape[0]
    u = np.asarray(u, dtype=np.float64).reshape(T, -1)
    m = u.shape[1]
    steps = np.arange(1, T)
    if update_hor is None:
        ush = u
    else:
        ush = np.vstack([u[1:], np.zeros((1, m))])      # u(i+1) at step i (the last row is never read)
        steps = steps[steps % int(update_hor) == 0]
    zpad = np.vstack([np.zeros((hor - 1, zeta.shape[1])), zeta])
    upad = np.vstack([np.zeros((hor - 1, m)), ush])
    return zpad, upad, steps


def assemble_val_observer(T, nw, steps, est, resnorm=None, sparse=False):
    """what (T x nw) of a trial from the estimates est[k] of steps[k] (as plan_val_observer returns them): what(1) = 0 and
    what(i+1) = the estimate of step i (:2043, :2061); sparse: what(i+1) = the mean of all estimates up to step i and
    res(i+1) = resnorm + 1e-6 at the estimated steps, both held in between, res(1) = 1e-6 (:2097, :2117-2134).
    Returns what, or (what, res) when sparse."""
    what = np.zeros((T, nw))
    est = np.asarray(est, dtype=np.float64).reshape(len(steps), nw)
    if not sparse:
        what[np.asarray(steps, dtype=np.int64)] = est
        return what
    res = np.full(T, 1e-6)
    at = {int(i): k for k, i in enumerate(steps)}
    total = np.zeros(nw)
    for i in range(1, T):
        k = at.get(i)
        if k is None:
            what[i], res[i] = what[i - 1], res[i - 1]
        else:
            total = total + est[k]
            what[i] = total / (k + 1)
            res[i] = resnorm[k] + 1e-6
    return what, res
