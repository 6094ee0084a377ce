"""Prediction-horizon validation, the parts that need no GPU.

* tests/_horizon_reference.py - the numpy restatement the GPU tests compare with, vectorised over the starts - against a plain
  loop of the oracle's one-step maps (econ_full, A z + B u, beta_bilinear, nl_step), start by start and step by step, on the toy
  trials of tests/_loaded_system.make_trials: the three model types, delays 0 and 1, with and without dim_red.  Both sides are
  f64 numpy with differently ordered sums.  Tolerance: one step rounds a prediction by at most K eps max|M| max|z| - K <= 45
  terms, |z| <= 10, so 1e-13 max|M| - and at most 8 steps follow one another, with predictions that stay bounded: 1e-12
  max(1, ||M||_2) absolute, M = [A B] or Kf (the delay-embedded least-squares fits on these few samples have entries in the
  thousands; the fits without delays have ||M|| = 1.07 and are held to 1.1e-12).
* kp_validate_horizon declared in include/koopman_hip_horizon.h, exported by the built library and bound in _ffi.
* Ksysid.horizon_slice and select_model(horizon=...) on hand-made tables."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd.ksysid import Ksysid
from oracle import koopman_oracle as ko
from tests import _horizon_reference as hr
from tests._loaded_system import make_trials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _toy(mt, nd, dim_red):
    trials = [{k: np.asarray(x) for k, x in t.items() if k != "w"} for t in make_trials(6, 60, nw=1, seed=4)]
    n, m = 2, 1
    pairs = ko.snapshot_pairs(ko.merge_trials(trials[:4]), nd)
    nzeta = n + nd * (n + m)
    dic = ko.build_dictionary(mt, nzeta, m, ["poly"], [2], pairs=pairs, dim_red=dim_red)
    koop = ko.get_koopman(dic, pairs)
    model = {"linear": ko.get_model, "bilinear": ko.get_blmodel, "nonlinear": ko.get_nlmodel}[mt](dic, koop, n)
    val = [ko.get_zeta(v["y"], v["u"], nd) for v in trials[4:]]
    return dic, model, val, n, m


def _loop(dic, model, Zeta, U, n, H, stride):
    """The definition, one start and one step at a time, by the oracle's one-step maps."""
    mt, T = dic.model_type, Zeta.shape[0]
    out = []
    s = 0
    while s + H <= T - 1:
        ys = []
        if mt == "nonlinear":
            z = Zeta[s].copy()
            for h in range(H):
                z = ko.nl_step(dic, model, z, U[s + h])
                ys.append(z[:n])
        else:
            z = ko.econ_full(dic, Zeta[s][None, :])[0]
            for h in range(H):
                if mt == "bilinear":
                    z = model["A"] @ z + ko.beta_bilinear(model["B"], z, dic.m) @ U[s + h]
                else:
                    z = model["A"] @ z + model["B"] @ U[s + h]
                ys.append(z[:n])
        out.append((s, np.array(ys)))
        s += stride
    return out


@pytest.mark.parametrize("dim_red", [False, True])
@pytest.mark.parametrize("nd", [0, 1])
@pytest.mark.parametrize("mt", ["linear", "bilinear", "nonlinear"])
def test_the_restatement_is_the_loop_of_one_step_maps(mt, nd, dim_red):
    dic, model, val, n, m = _toy(mt, nd, dim_red)
    assert (dic.pcs is not None) == dim_red
    fac = np.array([2.0, 0.5])
    for (Zeta, U), (H, stride) in zip(val, [(8, 1), (5, 3)]):
        ref = _loop(dic, model, Zeta, U, n, H, stride)
        got = hr.horizon_errors(dic, model, Zeta, U, n, fac, H, stride)
        assert got["starts"] == len(ref) == len(hr.starts(Zeta.shape[0], H, stride)) > 3
        assert [s for s, _ in ref] == list(hr.starts(Zeta.shape[0], H, stride)) and ref[-1][0] + H <= Zeta.shape[0] - 1 < ref[-1][0] + H + stride
        yl = np.array([y for _, y in ref])
        assert np.isfinite(yl).all() and np.abs(yl).max() < 10.0
        M = model["Kf"] if mt == "nonlinear" else np.hstack([model["A"], model["B"]])
        tol = 1e-12 * max(1.0, np.linalg.norm(M, 2))
        assert np.abs(got["yhat"] - yl).max() < tol
        d = np.array([y - Zeta[s + 1:s + H + 1, :n] for s, y in ref])          # S x H x n
        assert np.abs(got["mean"] - np.abs(d).mean(axis=0)).max() < 2.0 * tol
        assert np.abs(got["rmse"] - np.sqrt((d ** 2).sum(axis=0) / len(ref))).max() < 2.0 * tol
        eu = np.array([[np.linalg.norm(d[i, h]) for h in range(H)] for i in range(len(ref))])
        euu = np.array([[np.linalg.norm(d[i, h] * fac) for h in range(H)] for i in range(len(ref))])
        assert np.abs(got["euclid_mean"] - eu.mean(axis=0)).max() < 2.0 * tol
        assert np.abs(got["unscaled_euclid_mean"] - euu.mean(axis=0)).max() < 2.0 * tol
        assert got["mean"].shape == got["rmse"].shape == (H, n) and got["euclid_mean"].shape == (H,)


def test_a_trial_shorter_than_the_horizon_has_no_start():
    dic, model, val, n, _ = _toy("linear", 0, False)
    Zeta, U = val[0]
    got = hr.horizon_errors(dic, model, Zeta[:8], U[:8], n, 1.0, 8)
    assert got["starts"] == 0 and np.isnan(got["mean"]).all() and np.isnan(got["euclid_mean"]).all()
    one = hr.horizon_errors(dic, model, Zeta[:9], U[:9], n, 1.0, 8)
    assert one["starts"] == 1 and np.isfinite(one["rmse"]).all()


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def _declaration():
    text = open(os.path.join(ROOT, "include", "koopman_hip_horizon.h")).read()
    m = re.search(r"^int\s+kp_validate_horizon\s*\(([^;]*)\)\s*;", text, re.M)
    assert m, "kp_validate_horizon is not declared in koopman_hip_horizon.h"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_declared_in_the_header():
    names = [a.split()[-1].lstrip("*") for a in _declaration()]
    assert names == ["ctx", "basis", "model_type", "N", "m", "n", "nzeta", "nmod", "A", "B", "ntr", "trial_off", "Zeta", "U", "yfactor",
                     "H", "stride", "err_out", "nstart_out", "status_out"]


def test_exported_by_the_library():
    assert hasattr(C.CDLL(F.LIB_PATH), "kp_validate_horizon")


def test_bound_with_the_declared_argument_types():
    res, argtypes = F.HORIZON_SIGNATURES["kp_validate_horizon"]
    assert res is C.c_int

    def ctype(decl):
        if decl.startswith("kp_ctx*") or decl.startswith("const kp_basis*"):
            return F.vp
        if "int64_t*" in decl:
            return C.POINTER(C.c_int64)
        if "double*" in decl:
            return F.c_dp
        if "int*" in decl:
            return F.c_ip
        assert decl.startswith("int "), decl
        return C.c_int
    assert argtypes == [ctype(a) for a in _declaration()]
    assert getattr(F.lib(), "kp_validate_horizon").argtypes == argtypes
    assert (F.TIMER_HORIZON, F.TIMER_HORIZON_TILE) == (24, 25)
    text = open(os.path.join(ROOT, "include", "koopman_hip_horizon.h")).read()
    assert re.search(r"KP_HORIZON_CHUNK\s*=\s*%d\b" % F.HORIZON_CHUNK, text)
    # the timer slots are documented where the others are
    main = open(os.path.join(ROOT, "include", "koopman_hip.h")).read()
    block = main[:main.index("int kp_timer_get")]
    assert re.search(r"\b24: the two kernels of\s+\*?\s*the most recent prediction-horizon validation", block) and "25: not a time" in block


# ---- slicing and selection -----------------------------------------------------------------------------------------------
def _bare(ncand=3):
    ks = Ksysid.__new__(Ksysid)
    ks.candidates = [{"id": i} for i in range(ncand)]
    ks.model = ks.candidates[0]
    return ks


def _htable(nmod=3, starts=(5, 0, 2), H=4, n=2, seed=0):
    rng = np.random.default_rng(seed)
    ntr = len(starts)
    tab = {"mean": rng.uniform(0.1, 1.0, (nmod, ntr, H, n)), "rmse": rng.uniform(0.1, 1.0, (nmod, ntr, H, n)),
           "euclid_mean": rng.uniform(0.1, 1.0, (nmod, ntr, H)), "unscaled_euclid_mean": rng.uniform(0.1, 1.0, (nmod, ntr, H)),
           "starts": np.array(starts, dtype=np.int64), "diverged": np.zeros((nmod, ntr), dtype=bool), "horizon": H, "stride": 1,
           "lasso": np.arange(1.0, nmod + 1.0)}
    for k in ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean"):
        tab[k][:, np.array(starts) == 0] = np.nan
    return tab


def test_horizon_slice_has_the_shapes_of_a_val_candidates_table_and_drops_empty_trials():
    tab = _htable()
    sl = Ksysid.horizon_slice(tab, 3)
    assert set(sl) == {"mean", "rmse", "euclid_mean", "unscaled_euclid_mean", "diverged", "lasso"}
    assert sl["mean"].shape == sl["rmse"].shape == (3, 2, 2) and sl["euclid_mean"].shape == sl["diverged"].shape == (3, 2)
    for k in ("mean", "rmse", "euclid_mean", "unscaled_euclid_mean"):
        assert np.array_equal(sl[k], tab[k][:, [0, 2], 2]) and np.isfinite(sl[k]).all()
    assert np.array_equal(sl["lasso"], [1.0, 2.0, 3.0])
    assert np.array_equal(Ksysid.horizon_slice(tab, 1)["rmse"], tab["rmse"][:, [0, 2], 0])
    assert np.array_equal(Ksysid.horizon_slice(tab, 4)["euclid_mean"], tab["euclid_mean"][:, [0, 2], 3])
    del tab["lasso"]
    assert "lasso" not in Ksysid.horizon_slice(tab, 2)


def test_horizon_slice_refuses_steps_outside_the_horizon_and_tables_without_a_start():
    tab = _htable()
    for h in (0, 5, -1, 1.5):
        with pytest.raises(ValueError, match="1 .. 4"):
            Ksysid.horizon_slice(tab, h)
    with pytest.raises(ValueError, match="long enough"):
        Ksysid.horizon_slice(_htable(starts=(0, 0)), 2)


def test_select_model_takes_a_slice_and_ranks_by_the_step():
    ks = _bare()
    tab = _htable()
    tab["rmse"][:, :, 3] = 1.0
    tab["rmse"][1, [0, 2], 3] = 0.05                               # candidate 1 is best at step 4 only
    tab["rmse"][2, :, :3] = 0.01
    best, out = ks.select_model("rmse", table=Ksysid.horizon_slice(tab, 4))
    assert best == 1 and ks.model is ks.candidates[1] and out["rmse"].shape == (3, 2, 2)
    assert ks.select_model("rmse", table=Ksysid.horizon_slice(tab, 2))[0] == 2
    assert ks.select_model("rmse", table=Ksysid.horizon_slice(tab, 4), horizon=4)[0] == 1
    tab["diverged"][1, 2] = True                                    # diverged on a kept trial: last
    assert ks.select_model("rmse", table=Ksysid.horizon_slice(tab, 4))[0] != 1
    tab["diverged"][1] = [False, True, False]                       # diverged on the dropped trial only: does not count
    assert ks.select_model("rmse", table=Ksysid.horizon_slice(tab, 4))[0] == 1


def test_select_model_with_a_horizon_builds_the_slice_of_val_horizon_and_refuses_nrmse():
    ks = _bare()
    tab = _htable()
    tab["euclid_mean"][0, [0, 2], 2] = 0.01
    calls = []

    def stub(horizon, models=None, valdata=None, stride=1):
        calls.append((horizon, stride))
        return tab

    ks.val_horizon = stub
    best, out = ks.select_model(horizon=3, stride=2)
    assert calls == [(3, 2)] and best == 0 and np.array_equal(out["euclid_mean"], tab["euclid_mean"][:, [0, 2], 2])
    with pytest.raises(ValueError, match="nrmse"):
        ks.select_model("nrmse", horizon=3)
    with pytest.raises(ValueError, match="nrmse"):
        ks.select_model("nrmse", table=Ksysid.horizon_slice(tab, 3), horizon=3)
    assert calls == [(3, 2)]


def test_pooled_weights_the_trials_by_their_starts():
    tab = _htable(starts=(5, 0, 2))
    p = Ksysid._horizon_pool(tab)
    assert p["mean"].shape == p["rmse"].shape == (3, 4, 2) and p["euclid_mean"].shape == (3, 4)
    np.testing.assert_allclose(p["euclid_mean"], (5 * tab["euclid_mean"][:, 0] + 2 * tab["euclid_mean"][:, 2]) / 7, rtol=1e-15)
    np.testing.assert_allclose(p["rmse"], np.sqrt((5 * tab["rmse"][:, 0] ** 2 + 2 * tab["rmse"][:, 2] ** 2) / 7), rtol=1e-15)
    assert np.isnan(Ksysid._horizon_pool(_htable(starts=(0, 0)))["mean"]).all()


def test_val_horizon_declines_continuous_and_loaded_objects():
    ks = _bare()
    ks.time_type, ks.loaded = "continuous", False
    with pytest.raises(NotImplementedError, match="continuous"):
        ks.val_horizon(5)
    ks.time_type, ks.loaded = "discrete", True
    with pytest.raises(NotImplementedError, match="loaded"):
        ks.val_horizon(5)
