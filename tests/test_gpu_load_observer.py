"""The batched load observer on the device (kp_load_observe, Ksysid.observer_load / val_observer_load /
val_observer_load_sparse): window parity with the oracle's rows and lsqlin, agreement with the observer fused into
kp_mpc_step_loaded, whole-trial semantics against a literal transcription of the reference's loops, batching and
determinism, estimation quality, refusals and failed windows."""
import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from koopman_realizations_amd.observer import plan_val_observer
from oracle import koopman_oracle as ko
from tests._loaded_system import make_trials
from tests.test_load_observer_host import _host_observer, _literal

pytestmark = pytest.mark.gpu

_MODELS = {}


def loaded(mt, nw):
    """A loaded toy model fitted as in tests/test_gpu_loaded_loop.py (poly degree 2, nd = 0) and the oracle's dictionary."""
    if (mt, nw) not in _MODELS:
        trials = make_trials(10, 150, nw=nw, seed=7)
        ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, model_type=mt, obs_type=["poly"], obs_degree=[2], loaded=True)
        ks.train_models()
        dic = ko.build_dictionary(mt, ks.params["nzeta"], 1, ["poly"], [2])
        assert dic.N == ks.params["N"]
        _MODELS[(mt, nw)] = (ks, dic)
    return _MODELS[(mt, nw)]


def observe(ks, trials, win_trial, win_start, hor, whatpast=None, flags=0):
    return ks.ctx.load_observe(ks.basis_dev, ks.model_type, ks.model["A"], ks.model["B"], ks.params["nw"], trials, win_trial,
                               win_start, hor, whatpast, flags)


def _rows(ks, dic, zwin, uwin):
    """The regression rows and right-hand sides of a window (oracle lift, the observer_load reading)."""
    mt, nw, nz = ks.model_type, ks.params["nw"], dic.nzeta
    A, B, NL = ks.model["A"], ks.model["B"], dic.N * (nw + 1)
    rows, rhs = [], []
    for k in range(zwin.shape[0] - 1):
        Om = np.kron(np.eye(nw + 1), ko.econ_full(dic, zwin[k][None, :])[0][:, None])
        R = A[:nz] @ Om
        if mt == "linear":
            rhs.append(zwin[k + 1, :nz] - B[:nz] @ uwin[k])
        else:
            R = R + B[:nz, :NL] @ Om * uwin[k, 0]
            rhs.append(zwin[k + 1, :nz])
        rows.append(R)
    return np.vstack(rows), np.concatenate(rhs)


@pytest.mark.parametrize("mt,nw", [("linear", 1), ("linear", 2), ("linear", 3), ("bilinear", 1), ("bilinear", 2)])
def test_every_window_matches_the_oracle(mt, nw):
    ks, dic = loaded(mt, nw)
    for hor in (2, 3, 11, 40):
        plans = [plan_val_observer(v["y"], v["u"], hor) for v in ks.valdata[:2]]
        wt = np.concatenate([np.full(len(p[2]), q) for q, p in enumerate(plans)])
        wsx = np.concatenate([p[2] - 1 for p in plans])
        what, res, st = observe(ks, [(p[0], p[1]) for p in plans], wt, wsx, hor)
        nfail = nill = ncmp = 0
        for w in range(len(wt)):
            zp, up, _ = plans[wt[w]]
            s = wsx[w]
            Cl, dl = _rows(ks, dic, zp[s:s + hor], up[s:s + hor])
            sv = np.linalg.svd(Cl[:, 1:], compute_uv=False)
            if st[w] != 0:
                # a failed window is one whose rows do not determine the loads (the zero-padded first windows with nw > nz):
                # a pivot under 1e-8 of its diagonal entry means sigma_min / sigma_max <= 1e-4 (1e-3: rounding)
                assert len(sv) < nw or sv[-1] <= 1e-3 * sv[0], (hor, w, sv)
                assert np.isnan(what[w]).all() and np.isnan(res[w])
                nfail += 1
                continue
            assert len(sv) == nw, (hor, w)
            if sv[-1] <= 1e-3 * sv[0]:
                # cond > 1e3 (cond(H) > 1e6): the dual active-set iteration works with H^-1, and the estimate moves by
                # more than 1e-8 with the rounding (measured 3e-6 at cond 5e3, three active bounds): not compared
                nill += 1
                continue
            ncmp += 1
            if mt == "linear":
                ow, orn = ko._lsqlin_load(Cl, dl, nw, None, pin_last_zero=False)
            else:
                ow, orn = ko.estimate_load_bilinear(dic, ks.model, zp[s:s + hor], up[s:s + hor], nw, 0)
            # both solvers meet an active box row to their feasibility threshold, not exactly: that slack is admitted on
            # top of 1e-8; the residual norm's sensitivity grows with cond^2 of the free rows
            slack = max(0.0, np.abs(ow).max() - 1.0, np.abs(what[w]).max() - 1.0)
            kappa = sv[0] / sv[-1]
            assert np.abs(what[w] - ow).max() <= 1e-8 + 4.0 * slack, (hor, w, what[w], ow)
            floor = (1e-14 * np.linalg.norm(dl) * kappa) ** 2          # an exact fit: resnorm is rounding of ||d||
            assert abs(res[w] - orn) <= 1e-10 * max(1.0, (kappa / 100.0) ** 2) * orn + floor, (hor, w, res[w], orn, kappa)
        if nw > ks.params["nzeta"]:
            assert nfail > 0
        if hor >= 11:
            assert ncmp >= 0.9 * len(wt), (hor, ncmp, nill, nfail)


@pytest.mark.parametrize("mt,nw", [("linear", 2), ("bilinear", 1), ("bilinear", 2)])
def test_agrees_with_the_fused_step(mt, nw):
    """RATE and PIN_LAST: the same estimate and residual norm as kp_mpc_step_loaded's observer, up to 64 pairs."""
    ks, dic = loaded(mt, nw)
    mpc = kra.Kmpc(ks, horizon=8, input_bounds=[-1.0, 1.0], cost_running=1.0, cost_terminal=10.0, cost_input=0.01,
                   projmtx=ks.model["C"][:1])
    v = ks.valdata[0]
    ref = np.full((9, 1), 0.2)
    t = 100
    traj = {"y": v["y"][t:t + 1], "u": v["u"][t:t + 1]}
    pin = F.OBS_PIN_LAST if mt == "linear" and nw == 2 else 0
    for rows in (2, 11, 40, 65):
        yp, up = v["y"][t + 1 - rows:t + 1], v["u"][t + 1 - rows:t + 1]
        for wp in (None, np.zeros(nw), np.full(nw, 0.3)):
            _, _, fw = mpc.get_mpcInput_loaded(traj, ref, yp, up, estimate=True, whatpast=wp)
            flags = pin | (0 if wp is None else F.OBS_RATE)
            what, res, st = observe(ks, [(yp, up)], [0], [0], rows, None if wp is None else wp[None, :], flags)
            assert st[0] == 0
            assert np.abs(what[0] - fw).max() <= 1e-12, (rows, wp, what[0], fw)
            assert abs(res[0] - mpc.last_resnorm) <= 1e-12 * mpc.last_resnorm + 1e-28, (rows, wp, res[0], mpc.last_resnorm)


@pytest.mark.parametrize("mt,nw", [("linear", 1), ("linear", 2), ("bilinear", 2)])
def test_whole_trials_match_the_reference_loops(mt, nw):
    ks, dic = loaded(mt, nw)
    v = ks.valdata[1]
    for hor, uh in ((11, 3), (4, 1)):
        what, wreal, werr = ks.val_observer_load(hor, v)
        lw, _ = _literal(dic, ks.model, mt, nw, v["y"], v["u"], hor)
        assert np.abs(what - lw).max() <= 1e-8 and np.all(what[0] == 0)
        assert np.array_equal(wreal, v["w"]) and np.abs(werr - np.abs(v["w"] - lw)).max() <= 1e-8
        what, wreal, werr, res = ks.val_observer_load_sparse(hor, uh, v)
        lw, lr = _literal(dic, ks.model, mt, nw, v["y"], v["u"], hor, uh)
        assert np.abs(what - lw).max() <= 1e-8 and np.abs(werr - np.abs(v["w"] - lw)).max() <= 1e-8
        assert np.abs(res - lr).max() <= 1e-10 * np.abs(lr).max() and res[0] == 1e-6
    # observer_load: one window, with and without the rate rows
    yp, up = v["y"][20:31], v["u"][20:31]
    w1, r1 = ks.observer_load(yp, up)
    hw, hr = _host_observer(dic, ks.model, mt, nw, yp, up)
    assert np.abs(w1 - hw).max() <= 1e-8 and abs(r1 - hr) <= 1e-10 * hr + 1e-28
    w2, _ = ks.observer_load(yp, up, whatpast=np.full((2, nw), 0.5))
    assert np.abs(w2 - 0.5).max() <= 0.01 + 1e-12


def test_batches_are_bit_identical():
    ks, _ = loaded("bilinear", 2)
    v0, v1 = ks.valdata[0], ks.valdata[1]
    v1s = {k: v1[k][:97] for k in ("t", "y", "u", "w")}
    for hor in (11, 40):
        both = ks.val_observer_load_sparse(hor, 2, [v0, v1s])
        one = [ks.val_observer_load_sparse(hor, 2, v) for v in (v0, v1s)]
        for q in range(2):
            for a, b in zip((c[q] for c in both), one[q]):
                assert np.array_equal(a, b, equal_nan=True)
        again = ks.val_observer_load_sparse(hor, 2, [v0, v1s])
        for a, b in zip(both, again):
            for x, y in zip(a, b):
                assert np.array_equal(x, y, equal_nan=True)


def test_a_hundred_thousand_windows():
    """10^5 windows of hor = 101 (100 pairs each) in one call: every estimate finite and inside the box."""
    ks, _ = loaded("linear", 2)
    rng = np.random.default_rng(3)
    trials = [(rng.uniform(-1, 1, (1100, 2)), rng.uniform(-1, 1, (1100, 1))) for _ in range(100)]
    wt = np.repeat(np.arange(100), 1000)
    wsx = np.tile(np.arange(1000), 100)
    what, res, st = observe(ks, trials, wt, wsx, 101)
    assert what.shape == (100000, 2) and np.all(st == 0) and np.isfinite(res).all()
    assert np.all(np.abs(what) <= 1.0 + 1e-12)
    # the same windows in another order: the same numbers
    perm = rng.permutation(100000)[:5000]
    w2, r2, _ = observe(ks, trials, wt[perm], wsx[perm], 101)
    assert np.array_equal(w2, what[perm]) and np.array_equal(r2, res[perm])


def test_estimation_quality_on_a_constant_load():
    """Toy model, constant true load per trial, estimates after the first hor samples: the median |werr| of the device
    observer equals the host route's (a Python loop of per-window host solves), and stays under a bound calibrated on
    that host route: median |werr| = 0.03117 on the host route and 0.03117 on the device (bilinear, nw = 1, hor = 11,
    both validation trials); the bound is 0.05."""
    ks, dic = loaded("bilinear", 1)
    hor = 11
    errs, herrs = [], []
    for v in ks.valdata:
        _, _, werr = ks.val_observer_load(hor, v)
        errs.append(werr[hor:])
        hw = []
        for i in range(hor, len(v["t"])):
            hw.append(_host_observer(dic, ks.model, "bilinear", 1, v["y"][i - hor:i], v["u"][i - hor:i])[0])
        herrs.append(np.abs(v["w"][hor:] - np.array(hw)))
    med, hmed = float(np.median(np.concatenate(errs))), float(np.median(np.concatenate(herrs)))
    print(f"median |werr|: device {med:.4g}, host route {hmed:.4g}")
    assert abs(med - hmed) <= 1e-8
    assert med <= OBS_QUALITY_BOUND


OBS_QUALITY_BOUND = 0.05


def test_refusals():
    trials = make_trials(4, 60, nw=1, seed=1)
    data = {"train": trials[:3], "val": trials[3:]}
    ks0 = kra.Ksysid(data, model_type="linear", obs_type=["poly"], obs_degree=[2])
    with pytest.raises(ValueError, match="loaded"):
        ks0.val_observer_load(5, ks0.valdata[0])
    ksn = kra.Ksysid(data, model_type="nonlinear", obs_type=["poly"], obs_degree=[2], loaded=True)
    with pytest.raises(NotImplementedError):
        ksn.observer_load(trials[0]["y"][:5], trials[0]["u"][:5])
    ksd = kra.Ksysid(data, model_type="linear", obs_type=["poly"], obs_degree=[2], loaded=True, delays=1)
    with pytest.raises(ValueError, match="delays"):
        ksd.val_observer_load_sparse(5, 2, ksd.valdata[0])
    ks, _ = loaded("linear", 1)
    v = ks.valdata[0]
    with pytest.raises(ValueError, match="hor"):
        ks.val_observer_load(1, v)
    with pytest.raises(ValueError, match="hor"):
        ks.observer_load(v["y"][:1], v["u"][:1])
    with pytest.raises(ValueError, match="update_hor"):
        ks.val_observer_load_sparse(5, 0, v)
    with pytest.raises(ValueError, match="same number of rows"):
        ks.val_observer_load(5, {"t": v["t"], "y": v["y"], "u": v["u"][:-1], "w": v["w"]})
    with pytest.raises(ValueError, match="same number of rows"):
        ks.observer_load(v["y"][:5], v["u"][:4])
    # limits of the device call
    A, B = ks.model["A"], ks.model["B"]
    zp, up, steps = plan_val_observer(v["y"], v["u"], 5)
    with pytest.raises(F.KoopmanHipError, match="nw = 9") as e:
        ks.ctx.load_observe(ks.basis_dev, "linear", A, B, 9, [(zp, up)], [0], [0], 5)
    assert e.value.code == F.KP_ERR_ARG
    long_ = (np.zeros((1100, 2)), np.zeros((1100, 1)))
    with pytest.raises(F.KoopmanHipError, match="hor = 1026") as e:
        ks.ctx.load_observe(ks.basis_dev, "linear", A, B, 1, [long_], [0], [0], 1026)
    assert e.value.code == F.KP_ERR_ARG
    what, _, st = ks.ctx.load_observe(ks.basis_dev, "linear", A, B, 1, [long_], [0], [0], 1025)   # 1024 pairs: admitted
    assert st[0] == 0 or np.isnan(what).all()
    with pytest.raises(F.KoopmanHipError, match="outside its trial"):
        ks.ctx.load_observe(ks.basis_dev, "linear", A, B, 1, [(zp, up)], [0], [len(zp) - 4], 5)


def test_failed_windows_are_nan_and_their_neighbours_are_not():
    # zero-padded first windows of a model with nw = 3 > nz = 2 do not determine the loads
    ks, _ = loaded("linear", 3)
    v = ks.valdata[0]
    zp, up, steps = plan_val_observer(v["y"], v["u"], 3)
    what, res, st = observe(ks, [(zp, up)], np.zeros(len(steps), int), steps - 1, 3)
    assert st[0] == F.KP_ERR_QP_FAIL and np.isnan(what[0]).all() and np.isnan(res[0])
    assert np.all(st[1:] == 0) and np.isfinite(what[1:]).all() and np.isfinite(res[1:]).all()
    # a NaN sample fails exactly the windows whose pairs read it
    ks, _ = loaded("bilinear", 2)
    v = ks.valdata[0]
    hor = 11
    zp, up, steps = plan_val_observer(v["y"], v["u"], hor)
    zp = zp.copy()
    p = hor - 1 + 60
    zp[p, 1] = np.nan
    what, res, st = observe(ks, [(zp, up)], np.zeros(len(steps), int), steps - 1, hor)
    s = steps - 1
    hit = (s <= p) & (s + hor - 2 >= p - 1)
    assert hit.sum() == hor and np.all(st[hit] == F.KP_ERR_QP_FAIL) and np.isnan(what[hit]).all() and np.isnan(res[hit]).all()
    assert np.all(st[~hit] == 0) and np.isfinite(what[~hit]).all() and np.isfinite(res[~hit]).all()
