"""numpy restatement of prediction-horizon validation (kp_validate_horizon, include/koopman_hip_validate.h), vectorised over
the starts: one matrix product per horizon step over all starts of a trial.

Trial: Zeta (T x nzeta), the delay-embedded states after the nd shift, whose first n columns are the real outputs, and U
(T x m).  Starts s = 0, stride, 2 stride, ... while s + H <= T - 1.  From start s:
    linear     z_0 = econ_full(zeta_s), z_{h+1} = A z_h + B u_{s+h}                  yhat_{s,h} = z_h(1:n)
    bilinear   z_{h+1} = A z_h + sum_i u_{s+h,i} B_i z_h
    nonlinear  zeta_0 = zeta_s, zeta_{h+1} = Kf econ_full([zeta_h; u_{s+h}])         yhat = zeta(1:n)
and with d_{s,h} = yhat_{s,h} - y_{s+h}, per h = 1 .. H over the starts: mean |d| (n), rmse (n), the mean Euclidean norm of d
and of d .* yfactor."""
import numpy as np

from oracle import koopman_oracle as ko


def starts(T, H, stride):
    return np.arange(0, T - H, stride) if T - 1 >= H else np.zeros(0, dtype=int)


def predictions(dic, model, Zeta, U, n, H, stride=1):
    """yhat (S, H, n): the predictions of steps 1 .. H from every start, and the starts (S)."""
    Zeta = np.asarray(Zeta, dtype=np.float64); U = np.asarray(U, dtype=np.float64).reshape(Zeta.shape[0], -1)
    mt, m = dic.model_type, dic.m
    s = starts(Zeta.shape[0], H, stride)
    out = np.zeros((len(s), H, n))
    if len(s) == 0:
        return out, s
    with np.errstate(over="ignore", invalid="ignore"):
        if mt == "nonlinear":
            Kf = np.asarray(model["Kf"])
            z = Zeta[s].copy()                                             # S x nzeta
            for h in range(H):
                z = ko.econ_full(dic, np.hstack([z, U[s + h]])) @ Kf.T
                out[:, h] = z[:, :n]
            return out, s
        A, B = np.asarray(model["A"]), np.asarray(model["B"])
        N = A.shape[0]
        z = ko.econ_full(dic, Zeta[s])                                     # S x N
        for h in range(H):
            u = U[s + h]
            if mt == "bilinear":
                z = z @ A.T + sum(u[:, [i]] * (z @ B[:, i * N:(i + 1) * N].T) for i in range(m))
            else:
                z = z @ A.T + u @ B.T
            out[:, h] = z[:, :n]
    return out, s


def horizon_errors(dic, model, Zeta, U, n, yfactor, H, stride=1):
    """The figures of one (model, trial) pair: mean, rmse (H, n), euclid_mean, unscaled_euclid_mean (H), starts (count), yhat
    (S, H, n).  No start: NaN."""
    Zeta = np.asarray(Zeta, dtype=np.float64)
    yhat, s = predictions(dic, model, Zeta, U, n, H, stride)
    fac = np.broadcast_to(np.asarray(yfactor, dtype=np.float64), (n,))
    if len(s) == 0:
        nan = np.full((H, n), np.nan)
        return {"mean": nan, "rmse": nan.copy(), "euclid_mean": np.full(H, np.nan), "unscaled_euclid_mean": np.full(H, np.nan),
                "starts": 0, "yhat": yhat}
    yreal = np.stack([Zeta[s + h + 1, :n] for h in range(H)], axis=1)     # S x H x n
    with np.errstate(over="ignore", invalid="ignore"):
        d = yhat - yreal
        return {"mean": np.abs(d).mean(axis=0), "rmse": np.sqrt((d ** 2).mean(axis=0)),
                "euclid_mean": np.sqrt((d ** 2).sum(axis=2)).mean(axis=0),
                "unscaled_euclid_mean": np.sqrt(((d * fac) ** 2).sum(axis=2)).mean(axis=0), "starts": len(s), "yhat": yhat}


def horizon_table(dic, models, trials, n, yfactor, H, stride=1):
    """The table of val_horizon without `pooled`: trials a list of (Zeta, U)."""
    res = [[horizon_errors(dic, mo, Z, U, n, yfactor, H, stride) for Z, U in trials] for mo in models]
    tab = {k: np.array([[r[k] for r in row] for row in res]) for k in ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean")}
    tab["starts"] = np.array([r["starts"] for r in res[0]])
    return tab, res
