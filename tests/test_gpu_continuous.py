"""Continuous-time models on the device: kp_logm against scipy's logm, the ode45 rollouts (kp_rollout_ct / kp_rollout_nl_ct)
against the host dopri45 restatement and the exact zero-order-hold solution, and Ksysid(time_type='continuous') end to end."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from _ct_reference import (arm_trials, bilinear_rhs, continuous_K, discrete_recursion, linear_rhs, nonlinear_rhs, rollout_host,
                           zoh_recursion)

pytestmark = pytest.mark.gpu
scipy_linalg = pytest.importorskip("scipy.linalg")


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _random(n, upper, seed):
    rng = np.random.default_rng(seed)
    A = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    if upper:
        A = A + np.triu(rng.standard_normal((n, n)), 1) / np.sqrt(n)     # non-normal, every eigenvalue off the negative axis
    return A


def _arm_K(arm, mt, dim_red=True):
    dic = ko.build_dictionary(mt, 6, 3, ["poly"], [3], arm["pairs"], dim_red=dim_red)
    Px, Py = ko.px_py(dic, arm["pairs"])
    return dic, ko.koopman_ls(Px, Py)


# ---- 1. kp_logm against scipy ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 16, 37, 64, 127, 128, 129, 136, 250, 336, 512])
@pytest.mark.parametrize("upper", [False, True])
def test_logm_matches_scipy(ctx, n, upper):
    A = _random(n, upper, 100 + n)
    L, nsq, st = ctx.logm(A)
    assert st == F.KP_OK
    Lref = np.real(scipy_linalg.logm(A))
    assert _rel(L, Lref) <= (3e-11 if n > 256 else 1e-11), (_rel(L, Lref), nsq)


def test_logm_batch_of_mixed_conditioning_equals_single_calls(ctx):
    n = 40
    mats = [_random(n, False, 1), _random(n, True, 2), np.eye(n) + 1e-3 * _random(n, False, 3), 5.0 * _random(n, True, 4),
            np.diag(np.linspace(1e-3, 1e3, n)) + np.triu(_random(n, False, 5), 1)]
    Lb, nsb, stb = ctx.logm(np.stack(mats), 1e-12, 0.5)
    for i, A in enumerate(mats):
        L, nsq, st = ctx.logm(A, 1e-12, 0.5)
        assert st == stb[i] == F.KP_OK and nsq == nsb[i]
        assert np.array_equal(L, Lb[i])                        # bitwise: a matrix's result does not depend on the batch
        Lref = 0.5 * np.real(scipy_linalg.logm(A + 1e-12 * np.eye(n)))
        assert _rel(L, Lref) <= 1e-11


@pytest.mark.parametrize("mt, transpose", [("linear", True), ("bilinear", True), ("nonlinear", False)])
def test_logm_of_the_arm_koopman_matrices(ctx, arm, mt, transpose):
    _, K = _arm_K(arm, mt)
    A = K.T if transpose else K
    L, nsq, st = ctx.logm(A, 1e-12, 1.0)
    assert st == F.KP_OK
    Lref = np.real(scipy_linalg.logm(A + 1e-12 * np.eye(A.shape[0])))
    assert _rel(L, Lref) <= 1e-11, (_rel(L, Lref), nsq)


# ---- 2. hard cases and refusals -------------------------------------------------------------------------------------------
def test_logm_of_the_rank_deficient_arm_K(ctx, arm):
    _, K = _arm_K(arm, "bilinear", dim_red=False)
    assert K.shape == (336, 336)
    A = K.T
    L, nsq, st = ctx.logm(A, 1e-12, 1.0)
    if st == F.KP_OK:
        res = np.abs(scipy_linalg.expm(L) - (A + 1e-12 * np.eye(336))).max() / np.abs(A).max()
        assert res <= 1e-5, res
    else:
        assert st == F.KP_ERR_NOT_CONVERGED and np.isnan(L).all()


def test_logm_refuses_what_has_no_real_logarithm(ctx):
    A = _random(8, False, 7)
    A[:, 0] = 0.0; A[0, 0] = -1.0                          # eigenvalue -1 (A is block triangular)
    L, _, st = ctx.logm(A)
    assert st == F.KP_ERR_NOT_CONVERGED and np.isnan(L).all()
    B = np.diag([-1.0, -2.0, 1.0, 1.5])                    # det > 0, still no real logarithm
    L, _, st = ctx.logm(B)
    assert st == F.KP_ERR_NOT_CONVERGED and np.isnan(L).all()
    N = _random(6, False, 8); N[2, 3] = np.nan
    L, _, st = ctx.logm(N)
    assert st != F.KP_OK and np.isnan(L).all()
    with pytest.raises(F.KoopmanHipError) as e:
        ctx.logm(np.eye(513))
    assert e.value.code == F.KP_ERR_ARG
    # a failing matrix does not touch its neighbours in the batch
    Lb, _, stb = ctx.logm(np.stack([_random(8, False, 9), A]))
    assert list(stb) == [F.KP_OK, F.KP_ERR_NOT_CONVERGED]
    assert np.array_equal(Lb[0], ctx.logm(_random(8, False, 9))[0])


# ---- 3. Ksysid models -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ct_models(ctx, golden):
    train, val = arm_trials(golden)
    out = {}
    for mt in ("linear", "bilinear", "nonlinear"):
        ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type=mt, obs_type=["poly"], obs_degree=[3], dim_red=True,
                        time_type="continuous")
        ks.train_models()
        out[mt] = ks
    return out


def test_ksysid_continuous_models_match_a_scipy_restatement(ct_models, arm):
    for mt, ks in ct_models.items():
        p = ks.params; N, nz = p["N"], p["nzeta"]
        Kc = continuous_K(ks.koopData["K"], p["Ts"])
        mdl = ks.model
        if mt == "nonlinear":
            assert _rel(mdl["Kf"], Kc[:, :nz].T) <= 1e-10
            dic = ko.Dictionary("nonlinear", 6, 3, ko.make_basis(9, ["poly"], [3]), ks.basis["pcs"])
            zeta, u = np.full(6, 0.1), np.array([0.2, -0.1, 0.3])
            f = mdl["F_func"](zeta, u)
            np.testing.assert_allclose(f, Kc[:, :nz].T @ ko.econ_full(dic, np.concatenate([zeta, u]))[0], rtol=1e-9, atol=1e-12)
            continue
        UT = Kc.T
        assert _rel(mdl["A"], UT[:N, :N]) <= 1e-10
        assert _rel(mdl["B"], UT[:N, N:]) <= 1e-10
        if mt == "linear":
            # M = (L \ R)' with L = A Px + B U, R = Py (Ksysid.m:1206-1217), the oracle's rows on the device's axes
            dic = ko.Dictionary("linear", 6, 3, ko.make_basis(6, ["poly"], [3]), ks.basis["pcs"])
            Px, Py = ko.px_py(dic, arm["pairs"])
            # (the constant observable has a zero derivative, so L is numerically rank deficient and M is not determined - the
            #  reference's `L \ R` warns and returns a basic solution: M must solve the least-squares problem as well as lstsq's)
            Lm = Px @ Kc[:, :N]
            M = np.linalg.lstsq(Lm, Py[:, :N], rcond=None)[0].T
            r_dev = np.linalg.norm(Lm @ mdl["M"].T - Py[:, :N]); r_ref = np.linalg.norm(Lm @ M.T - Py[:, :N])
            assert r_dev <= (1 + 1e-5) * r_ref, (r_dev, r_ref)     # kp_model_project: normal equations (measured 1 + 2.8e-6)


# ---- 4. continuous validation ---------------------------------------------------------------------------------------------
def _val_inputs(ks):
    v = ks.valdata[0]
    t, yreal, ureal, zetareal = ks._val_common(v)
    return yreal, ureal, zetareal


def test_linear_val_model_equals_the_discrete_unprojected_recursion(ct_models):
    ks = ct_models["linear"]
    ks.ode_rtol, ks.ode_atol = 1e-10, 1e-12
    try:
        res = ks.val_model(ks.model, ks.valdata[0])
    finally:
        ks.ode_rtol, ks.ode_atol = 1e-3, 1e-6
    yreal, ureal, zetareal = _val_inputs(ks)
    N = ks.params["N"]
    KT = ks.koopData["K"].T
    Zd = discrete_recursion(KT[:N, :N], KT[:N, N:], ks.lift.econ_full(zetareal[0]), ureal)
    assert _rel(res["sim"]["y"][1:], Zd[1:, :6]) <= 1e-8


@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_device_rollout_matches_host_dopri45(ctx, ct_models, mt):
    ks = ct_models[mt]
    Ts = ks.params["Ts"]
    yreal, ureal, zetareal = _val_inputs(ks)
    mdl = ks.model
    if mt == "nonlinear":
        T = 100
        dic = ko.Dictionary("nonlinear", 6, 3, ko.make_basis(9, ["poly"], [3]), ks.basis["pcs"])
        Zh, na, nr = rollout_host(nonlinear_rhs(dic, mdl["Kf"]), zetareal[0], ureal[:T], Ts)
        Z, na_d, nr_d, st = ctx.rollout_nl_ct(ks.basis_dev, mdl["Kf"], zetareal[0], ureal[:T], Ts)
        Yd, Yh = Z[:, :6], Zh[:, :6]
        full = ks.val_NLmodel(mdl, ks.valdata[0])["sim"]["y"]
        assert np.array_equal(full[:T], Yd)
    else:
        z0 = ks.lift.econ_full(zetareal[0])
        rhs = linear_rhs if mt == "linear" else bilinear_rhs
        Zh, na, nr = rollout_host(rhs(mdl["A"], mdl["B"]), z0, ureal, Ts)
        Yd, na_d, nr_d, st = ctx.rollout_ct(mt, mdl["A"], mdl["B"], z0, ureal, 6, Ts)
        Yh = Zh[:, :6]
        val = (ks.val_model if mt == "linear" else ks.val_BLmodel)(mdl, ks.valdata[0])["sim"]["y"]
        assert np.array_equal(val[1:], Yd[1:]) and np.array_equal(val[0], yreal[0])
    assert st == F.KP_OK
    assert (na_d, nr_d) == (na, nr)
    assert _rel(Yd, Yh) <= 1e-10, _rel(Yd, Yh)


def test_tight_linear_rollout_matches_the_exact_zoh_solution(ctx, ct_models):
    ks = ct_models["linear"]
    yreal, ureal, zetareal = _val_inputs(ks)
    A, B = ks.model["A"], ks.model["B"]
    z0 = ks.lift.econ_full(zetareal[0])
    Y, na, nr, st = ctx.rollout_ct("linear", A, B, z0, ureal, A.shape[0], ks.params["Ts"], 1e-10, 1e-12)
    assert st == F.KP_OK
    Zx = zoh_recursion(A, B, z0, ureal, ks.params["Ts"])
    assert _rel(Y, Zx) <= 1e-8


def test_linear_continuous_validation_with_delays(ctx, golden):
    """Delays (nd = 1) in continuous-time validation: the delayed zeta, its lift and the ode45 rollout.  The fitted K of a
    delayed model has (near-)zero eigenvalues - the rows of the delayed inputs carry no state - so its logarithm is refused;
    the rollout is checked on a stable continuous model of the same shape against the host restatement."""
    train, val = arm_trials(golden)
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2], delays=1,
                    dim_red=True, time_type="continuous")
    with pytest.raises(F.KoopmanHipError):
        ks.train_models()
    N, m = ks.params["N"], ks.params["m"]
    rng = np.random.default_rng(11)
    model = {"A": -2.0 * np.eye(N) + rng.standard_normal((N, N)) / np.sqrt(N), "B": 0.5 * rng.standard_normal((N, m))}
    res = ks.val_model(model, ks.valdata[0])
    yreal, ureal, zetareal = _val_inputs(ks)
    assert zetareal.shape[1] == ks.params["nzeta"] == 6 * 2 + 3
    Zh, _, _ = rollout_host(linear_rhs(model["A"], model["B"]), ks.lift.econ_full(zetareal[0]), ureal, ks.params["Ts"])
    assert _rel(res["sim"]["y"][1:], Zh[1:, :6]) <= 1e-10
    assert np.isfinite(res["error"]["rmse"]).all()


# ---- 5. batching ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", ["linear", "bilinear"])
def test_rollout_batch_of_64_equals_single_calls(ctx, ct_models, mt):
    ks = ct_models[mt]
    yreal, ureal, zetareal = _val_inputs(ks)
    rng = np.random.default_rng(3)
    A, B = ks.model["A"], ks.model["B"]
    T = 120
    z0 = ks.lift.econ_full(zetareal[0])
    As = np.stack([A * (1 + 1e-3 * (i % 4)) for i in range(64)]); Bs = np.stack([B] * 64)
    Z0 = np.stack([z0 + 0.01 * rng.standard_normal(z0.size) * (i % 8) for i in range(64)])
    Us = np.stack([np.roll(ureal[:T], i, axis=0) for i in range(64)])
    Yb, nab, nrb, stb = ctx.rollout_ct(mt, As, Bs, Z0, Us, 6, ks.params["Ts"])
    for i in (0, 1, 17, 63):
        Y, na, nr, st = ctx.rollout_ct(mt, As[i], Bs[i], Z0[i], Us[i], 6, ks.params["Ts"])
        assert np.array_equal(Y, Yb[i]) and (na, nr, st) == (nab[i], nrb[i], stb[i])
    assert (stb == F.KP_OK).all()


def test_nonlinear_rollout_batch_equals_single_calls(ctx, ct_models):
    ks = ct_models["nonlinear"]
    yreal, ureal, zetareal = _val_inputs(ks)
    Kf = ks.model["Kf"]
    nb, T = 8, 40
    Kfs = np.stack([Kf * (1 + 1e-3 * i) for i in range(nb)])
    Z0 = np.stack([zetareal[i] for i in range(nb)])
    Us = np.stack([ureal[i:i + T] for i in range(nb)])
    Zb, nab, nrb, stb = ctx.rollout_nl_ct(ks.basis_dev, Kfs, Z0, Us, ks.params["Ts"])
    for i in (0, 5):
        Z, na, nr, st = ctx.rollout_nl_ct(ks.basis_dev, Kfs[i], Z0[i], Us[i], ks.params["Ts"])
        assert np.array_equal(Z, Zb[i]) and (na, nr, st) == (nab[i], nrb[i], stb[i])


def test_train_models_lasso_grid_equals_one_candidate_at_a_time(ctx, golden):
    train, val = arm_trials(golden)
    kw = dict(ctx=ctx, model_type="linear", obs_type=["poly"], obs_degree=[2], dim_red=True, time_type="continuous")
    las = [1e4, 2e4]
    grid = kra.Ksysid({"train": train, "val": val}, lasso=las, **kw).train_models()
    for lv, c in zip(las, grid.candidates):
        one = kra.Ksysid({"train": train, "val": val}, lasso=lv, **kw).train_models()
        for k in ("A", "B", "M"):
            assert np.array_equal(one.model[k], c[k]), k


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_loaded_continuous_and_mpc_of_a_continuous_model_are_refused(ctx, golden, ct_models):
    from tests._loaded_system import make_trials
    trials = make_trials(3, 100, nw=1, seed=2)
    with pytest.raises(NotImplementedError):
        kra.Ksysid({"train": trials[:2], "val": trials[2:]}, ctx=ctx, loaded=True, time_type="continuous")
    train, val = arm_trials(golden)
    with pytest.raises(ValueError):
        kra.Ksysid({"train": train, "val": val}, ctx=ctx, time_type="hybrid")
    with pytest.raises(ValueError):
        kra.Kmpc(ct_models["linear"], horizon=5)
