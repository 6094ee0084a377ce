"""Test-side restatement of the continuous-time models (Ksysid.m:1186-1187, 1245-1246, 1307-1310) and of their validation
(val_model :1679-1683, val_BLmodel :1777-1781, val_NLmodel :1849-1856): scipy's logm of the fitted K and the host `dopri45`
(arm.py, ode45's pair and step control) over every sample interval, the input held."""
import numpy as np

from koopman_realizations_amd.arm import dopri45
from oracle import koopman_oracle as ko


def arm_trials(golden):
    g = golden["arm_data"]
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    return train, val


def continuous_K(K, Ts):
    """(1/Ts) logm(K + 1e-12 I) by scipy (real part: the arm's K have real logarithms)."""
    from scipy.linalg import logm
    L = logm(np.asarray(K, dtype=np.float64) + 1e-12 * np.eye(K.shape[0]))
    return np.real(L) / Ts


def rollout_host(rhs, z0, U, Ts, rtol=1e-3, atol=1e-6, T=None):
    """ode45 over [0, Ts] per sample from the previous end point, input U[j] held; rows = samples.  Returns (Z, naccept,
    nreject)."""
    T = U.shape[0] if T is None else T
    Z = np.zeros((T, len(z0))); Z[0] = z0
    stats = {"naccept": 0, "nreject": 0}
    for j in range(T - 1):
        u = U[j]
        Z[j + 1] = dopri45(lambda t, z: rhs(z, u), 0.0, Ts, Z[j], rtol=rtol, atol=atol, stats=stats)
    return Z, stats["naccept"], stats["nreject"]


def linear_rhs(A, B):
    return lambda z, u: A @ z + B @ u


def bilinear_rhs(A, B):
    N, m = A.shape[0], B.shape[1] // A.shape[0]
    return lambda z, u: (A + sum(u[i] * B[:, i * N:(i + 1) * N] for i in range(m))) @ z


def nonlinear_rhs(dic, Kf):
    return lambda zeta, u: Kf @ ko.econ_full(dic, np.concatenate([zeta, u]))[0]


def zoh_recursion(A, B, z0, U, Ts):
    """Exact solution of z' = A z + B u with u held over each interval: z+ = Ad z + Bd u from expm of [[A, B], [0, 0]] Ts."""
    from scipy.linalg import expm
    N, m = B.shape
    E = expm(np.block([[A, B], [np.zeros((m, N + m))]]) * Ts)
    Ad, Bd = E[:N, :N], E[:N, N:]
    Z = np.zeros((U.shape[0], N)); Z[0] = z0
    for j in range(U.shape[0] - 1):
        Z[j + 1] = Ad @ Z[j] + Bd @ U[j]
    return Z


def discrete_recursion(A, B, z0, U):
    Z = np.zeros((U.shape[0], len(z0))); Z[0] = z0
    for j in range(U.shape[0] - 1):
        Z[j + 1] = A @ Z[j] + B @ U[j]
    return Z
