"""Nonlinear MPC (get_mpcInput_nonlinear, Kmpc.m:906-1181) on the host: the stored closed loop res_nonlin of
example_control.m (tests/golden/arm_nmpc.npz, written by make_golden_nmpc.py) and a single-shooting restatement of the
reference's fmincon problem that the device SQP (kp_nmpc_step) is checked against.

The restatement eliminates the states: z_0 = zeta, z_k = F(z_{k-1}, u_k) with F = Kf econ_full([zeta; u])
(get_NLmodel, Ksysid.m:1298-1341), u_1 = u_prev pinned (Aeq, :1149-1152), and minimises
  sum_{k=0..Np} q_k |C z_k - r_k|^2 + sum_k u_k' R u_k     (get_costMatrices_nonlinear, :909-943)
over u_2 .. u_Np with scipy's SLSQP under the linear rows of get_constraintMatrices_nonlinear (:946-1059) and the state
bounds, with exact gradients by the chain rule through the model's Jacobians (central differences of the oracle's
econ_full, exact to rounding for the poly-3 arm)."""
import os

import numpy as np
import pytest
from scipy.optimize import minimize

from oracle import koopman_oracle as ko

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_nmpc_golden():
    return np.load(os.path.join(GOLDEN, "arm_nmpc.npz"))


def fd_jacobian(dic, Kf, v, h=1e-2):
    """dF/dv (nzeta x nvars) at v by five-point central differences of the oracle's econ_full: exact for dictionaries of
    degree <= 4 in each variable (the poly-3 arm) up to rounding (~1e-14), O(h^4) otherwise."""
    nv = len(v)
    E = np.eye(nv)
    P = np.vstack([v + s * h * E for s in (2, 1, -1, -2)])
    F = ko.econ_full(dic, P) @ Kf.T
    f2, f1, m1, m2 = F[:nv], F[nv:2 * nv], F[2 * nv:3 * nv], F[3 * nv:]
    return ((-f2 + 8 * f1 - 8 * m1 + m2) / (12 * h)).T


class HostNmpc:
    """The reference's NMPC problem in the inputs only (single shooting), solved by SLSQP."""

    def __init__(self, dic, Kf, Np, proj, q_run, q_term, r, lo=None, hi=None, slope=None, smooth=None, sb_lo=None, sb_hi=None):
        self.dic, self.Kf, self.Np, self.C = dic, np.asarray(Kf), int(Np), np.atleast_2d(proj)
        self.q = np.array([q_run] * Np + [q_term], dtype=np.float64)
        self.r = np.asarray(r, dtype=np.float64)
        self.lo, self.hi, self.slope, self.smooth, self.sb_lo, self.sb_hi = lo, hi, slope, smooth, sb_lo, sb_hi
        self.nz, self.m = self.Kf.shape[0], len(self.r)

    def rollout(self, zeta, U, jac=False):
        Z = [np.asarray(zeta, dtype=np.float64)]
        Js = []
        for k in range(self.Np):
            v = np.concatenate([Z[-1], U[k]])
            Z.append(self.Kf @ ko.econ_full(self.dic, v[None, :])[0])
            if jac:
                Js.append(fd_jacobian(self.dic, self.Kf, v))
        return np.array(Z), Js

    def sens(self, Js):
        """S_k = dz_k / dU (nz x m Np), k = 0..Np."""
        nz, m, Np = self.nz, self.m, self.Np
        S = [np.zeros((nz, m * Np))]
        for k in range(1, Np + 1):
            A, B = Js[k - 1][:, :nz], Js[k - 1][:, nz:]
            Sk = A @ S[-1]
            Sk[:, (k - 1) * m:k * m] = B
            S.append(Sk)
        return S

    def cost(self, zeta, U, Yr):
        Z, _ = self.rollout(zeta, U)
        e = Z @ self.C.T - Yr.reshape(self.Np + 1, -1)
        return float((self.q * (e * e).sum(axis=1)).sum() + (self.r * U * U).sum())

    def solve(self, zeta, u_prev, Yr, tol=1e-14, maxiter=500, polish=True):
        m, Np = self.m, self.Np
        Yr = np.asarray(Yr).reshape(Np + 1, -1)
        cache = {}

        def full_U(x):
            return np.vstack([u_prev, x.reshape(Np - 1, m)])

        def evals(x):
            key = x.tobytes()
            if key not in cache:
                U = full_U(x)
                Z, Js = self.rollout(zeta, U, jac=True)
                cache.clear()
                cache[key] = (U, Z, self.sens(Js))
            return cache[key]

        def f(x):
            U, Z, S = evals(x)
            e = Z @ self.C.T - Yr
            J = (self.q * (e * e).sum(axis=1)).sum() + (self.r * U * U).sum()
            g = sum(2 * self.q[k] * (self.C @ S[k]).T @ e[k] for k in range(Np + 1)) + 2 * (self.r * U).ravel()
            return J, g[m:]

        cons = []
        D = []                       # linear rows on the full U (x layout), rhs
        if self.lo is not None:
            for j in range(Np):
                for i in range(m):
                    a = np.zeros(m * Np); a[j * m + i] = -1; D.append((a, -self.lo[i]))
                    a = np.zeros(m * Np); a[j * m + i] = 1; D.append((a, self.hi[i]))
        if self.slope is not None:
            for j in range(Np - 1):
                for i in range(m):
                    a = np.zeros(m * Np); a[j * m + i] = -1; a[(j + 1) * m + i] = 1
                    D.append((a, self.slope)); D.append((-a, self.slope))
        if self.smooth is not None:
            for j in range(Np - 2):
                for i in range(m):
                    a = np.zeros(m * Np); a[j * m + i] = 1; a[(j + 1) * m + i] = -2; a[(j + 2) * m + i] = 1
                    D.append((a, self.smooth)); D.append((-a, self.smooth))
        if D:
            A = np.array([d[0] for d in D]); b = np.array([d[1] for d in D])
            cons.append({"type": "ineq", "fun": lambda x: b - A @ full_U(x).ravel(), "jac": lambda x: -A[:, m:]})
        if self.sb_lo is not None:
            def sfun(x):
                _, Z, _ = evals(x)
                return np.concatenate([(Z - self.sb_lo).ravel(), (self.sb_hi - Z).ravel()])

            def sjac(x):
                _, _, S = evals(x)
                Sa = np.vstack(S)[:, m:]
                return np.vstack([Sa, -Sa])
            cons.append({"type": "ineq", "fun": sfun, "jac": sjac})
        x0 = np.tile(u_prev, Np - 1)                                         # X0 of Kmpc.m:1155
        res = minimize(f, x0, jac=True, method="SLSQP", constraints=cons, options={"ftol": tol, "maxiter": maxiter})
        res = minimize(f, res.x, jac=True, method="SLSQP", constraints=cons, options={"ftol": tol, "maxiter": maxiter})  # restart: fresh quasi-Newton matrix
        if polish:
            # SLSQP stops on the change of J, which leaves ~1e-6 in U along the weakly penalised inputs.  Polish from its
            # solution with full Gauss-Newton SQP steps (exact gradient, the constraints linearised, the oracle's QP
            # solver) until the step is at rounding level: the fixed point is the KKT point SLSQP approached.
            x = res.x.copy()
            for _ in range(100):
                U, Z, S = evals(x)
                J, g = f(x)
                Hgn = 2 * (sum(self.q[k] * (self.C @ S[k]).T @ (self.C @ S[k]) for k in range(Np + 1)) + np.diag(np.tile(self.r, Np)))
                G = np.vstack([-c["jac"](x) for c in cons]); gv = np.concatenate([c["fun"](x) for c in cons])   # G dx <= v
                dx, _, ok = ko.qp_solve(Hgn[m:, m:], g, G, gv)
                if not ok or not np.all(np.isfinite(dx)) or np.abs(dx).max() > 1e-3:
                    break
                x = x + dx
                if np.abs(dx).max() < 1e-14:
                    break
            res.x = x
        return full_U(res.x), res


def arm_nonlinear_model(golden_arm_data):
    """The oracle refit of example_sysid.m's nonlinear arm model (poly 3, dim_red: N = 88), scale and dictionary."""
    g = golden_arm_data
    data = {"t": g["train_t"], "y": g["train_y"], "u": g["train_u"]}
    sd, sc = ko.get_scale(data)
    pairs = ko.snapshot_pairs(sd, 0)                                      # (trial seams: the time stamps, Ksysid.m:941-948)
    dic = ko.build_dictionary("nonlinear", 6, 3, ["poly"], [3], pairs, dim_red=True)
    koop = ko.get_koopman(dic, pairs)
    mdl = ko.get_nlmodel(dic, koop, 6)
    return dic, mdl, sc


def test_fixture_matches_generator():
    d = load_nmpc_golden()
    assert d["Y"].shape == (301, 6) and d["U"].shape == (301, 3) and d["R"].shape == (301, 2) and d["X"].shape == (301, 6)
    assert d["err"].shape == (300, 1) and d["comp_time"].shape == (300, 1) and d["Z6"].shape == (300, 6)
    assert int(d["Zwidth"]) == 88
    assert float(d["Zpad_absmax"]) == 0.0                                # z = [zeta; zeros(N - n, 1)] (Kmpc.m:1180)
    assert np.allclose(d["err"].mean(), 0.01923, atol=5e-6)
    assert 1.0 < d["comp_time"].mean() < 1.5                             # fmincon: 1.16 s per step


@pytest.fixture(scope="module")
def arm_nl():
    g = np.load(os.path.join(GOLDEN, "arm_data.npz"))
    return arm_nonlinear_model(g)


def test_host_restatement_reproduces_stored_inputs(arm_nl):
    """Teacher-forced from the stored Y(k), U(k) and the reference rows k..k+10 (Ksim.m:153-166, :198-202), the
    single-shooting problem gives the stored U(k+1) (Ksim.m:225) of steps k = 1..3 to 1e-6: the oracle refit is the model
    behind the stored run, input_bounds = [] and input_slopeConst = 1e-1 its settings."""
    dic, mdl, sc = arm_nl
    d = load_nmpc_golden()
    ref = np.load(os.path.join(GOLDEN, "blockM_ref.npz"))["y"]
    ysc = lambda y: ko.scaledown(sc, "y", y)
    usc = lambda u: ko.scaledown(sc, "u", u)
    proj = np.eye(6)[-2:]
    ref_sc = (ref - sc["y_offset"][-2:]) / sc["y_factor"][-2:]
    host = HostNmpc(dic, mdl["Kf"], 10, proj, 10.0, 100.0, 0.1 * np.array([3e-2, 2e-2, 1e-2]),
                    slope=1e-1 * sc["u_factor"].mean())
    for k in range(3):
        U, res = host.solve(ysc(d["Y"][k]), usc(d["U"][k]), ref_sc[k:k + 11].ravel())
        dev = np.abs(ko.scaleup(sc, "u", U[1]) - d["U"][k + 1]).max()
        assert dev < 1e-6, (k, dev, res.message)
