"""Loaded closed loops on the device: kp_mpc_step_loaded (the load observer, the loaded lift and the MPC step in one
launch) against the oracle's estimate_load_* / loaded_lift / QP, its gateway form, the reference's circle runs run
free under plant loads, and a loaded closed loop end to end.  The reference ships no loaded model of its own, so the
loaded step's parity is with the oracle only."""
import os

import numpy as np
import pytest

import koopman_realizations_amd as kra
from koopman_realizations_amd import _ffi as F
from oracle import koopman_oracle as ko
from tests._loaded_system import _step as toy_step, make_trials

pytestmark = pytest.mark.gpu

_MODELS = {}


def loaded_model(mt, nw, nd):
    """A loaded model fitted as in tests/test_loaded.py, its controller and the oracle's dictionary."""
    key = (mt, nw, nd)
    if key not in _MODELS:
        trials = make_trials(10, 150, nw=nw, seed=7)
        ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, model_type=mt, obs_type=["poly"], obs_degree=[2], loaded=True,
                        delays=nd)
        ks.train_models()
        mpc = kra.Kmpc(ks, horizon=8, input_bounds=[-1.0, 1.0], input_slopeConst=0.5, cost_running=1.0, cost_terminal=10.0,
                       cost_input=0.01, projmtx=ks.model["C"][:1])
        dic = ko.build_dictionary(mt, ks.params["nzeta"], 1, ["poly"], [2])
        assert dic.N == ks.params["N"]
        sc = ks.params["scale"]
        s = ko.MpcSetup(model_type=mt, A=ks.model["A"], B=ks.model["B"], m=1, Np=8, projmtx=ks.model["C"][:1], cost_running=1.0,
                        cost_terminal=10.0, cost_input=np.array([0.01]),
                        input_bounds=np.stack([(np.array([-1.0]) - sc["u_offset"]) / sc["u_factor"],
                                               (np.array([1.0]) - sc["u_offset"]) / sc["u_factor"]], axis=1),
                        slope_lim=0.5 * float(np.mean(sc["u_factor"])), smooth_lim=None, n=2)
        _MODELS[key] = (ks, mpc, dic, s)
    return _MODELS[key]


@pytest.mark.parametrize("nd", [0, 1])
@pytest.mark.parametrize("mt,nw", [("linear", 2), ("bilinear", 1), ("bilinear", 2)])
def test_fused_loaded_step_matches_the_oracle(mt, nw, nd):
    ks, mpc, dic, s = loaded_model(mt, nw, nd)
    oest = ko.estimate_load_linear if mt == "linear" else ko.estimate_load_bilinear
    v = ks.valdata[0]
    ref = np.full((9, 1), 0.2)
    t = 60
    traj = {"y": v["y"][t - nd:t + 1], "u": v["u"][t - nd:t + 1]}
    zeta = ks.get_zeta(traj)[1][-1]
    for rows in (nd + 2, 11, 40):
        yp, up = v["y"][t + 1 - rows:t + 1], v["u"][t + 1 - rows:t + 1]
        for wp in (None, np.zeros(nw), np.full(nw, 0.3)):
            U, z, what = mpc.get_mpcInput_loaded(traj, ref, yp, up, estimate=True, whatpast=wp)
            owhat, orn = oest(dic, ks.model, yp, up, nw, nd, wp)
            assert np.abs(what - owhat).max() <= 1e-8, (rows, wp, what, owhat)
            assert abs(mpc.last_resnorm - orn) <= 1e-10 * orn + 1e-28, (rows, wp, mpc.last_resnorm, orn)   # (0 for an exact fit)
            if mt == "linear":
                assert what[-1] == 0.0                                   # the debugging pin of Kmpc.m:1350
            free = nw - 1 if mt == "linear" and nw == 2 else nw
            if wp is not None:
                assert np.abs(what - wp)[:free].max() <= 0.01 + 1e-12    # rate rows (Kmpc.m:1344-1347)
            zo = ko.loaded_lift(ko.econ_full(dic, zeta[None, :]), what[None, :])[0]
            assert np.abs(z - zo).max() <= 1e-13
            Hr, fr, Ar, br = ko.mpc_qp(s, zo, traj["u"][-1], ref)
            x, _, ok = ko.qp_solve(Hr, fr, Ar, br)
            assert ok and np.abs(U.reshape(-1) - x).max() <= 1e-8
    # nobs = 0: no estimate, the lift takes traj['what'] - the host path's step
    traj["what"] = np.full((1, nw), 0.25)
    U0, z0, w0 = mpc.get_mpcInput_loaded(traj, ref, None, None, estimate=False)
    Uh, zh = mpc._step(traj, ref, 1)
    assert np.array_equal(w0, traj["what"][0]) and np.abs(z0 - zh).max() <= 1e-13 and np.abs(U0 - Uh).max() <= 1e-10


@pytest.mark.parametrize("mt,nw", [("linear", 2), ("bilinear", 1)])
def test_fused_loaded_step_with_state_bounds_and_iters(mt, nw):
    """The loaded step with state bounds (Kmpc.m:300-318, the multi-pass path: assembly, the dense constraint rows, the
    generic QP kernel) and iters > 1 (Kmpc.m:874-899): against the oracle's estimate, lift and iterated QP with the state
    rows, and against the unfused step on the same lifted state.  (The reference's state rows bound the first (Np + 1) n
    entries of the stacked lifted state, kp_mpc_set_state_bounds; what is pinned here is that the loaded step assembles
    and solves the same problem as the oracle and the unfused step.)  A failed estimate fails the step on this path too, and
    the next step (its warm start) is unaffected."""
    trials = make_trials(10, 150, nw=nw, seed=7)
    ks = kra.Ksysid({"train": trials[:8], "val": trials[8:]}, model_type=mt, obs_type=["poly"], obs_degree=[2], loaded=True)
    ks.train_models()
    sc = ks.params["scale"]
    sb_sc = np.array([[-0.6, 0.15], [-1.5, 1.5]])                        # scaled bounds of the two outputs
    sb = sb_sc * sc["y_factor"][:, None] + sc["y_offset"][:, None]
    mpc = kra.Kmpc(ks, horizon=8, input_bounds=[-1.0, 1.0], input_slopeConst=0.5, cost_running=1.0, cost_terminal=10.0,
                   cost_input=0.01, projmtx=ks.model["C"][:1], state_bounds=sb)
    dic = ko.build_dictionary(mt, 2, 1, ["poly"], [2])
    s = ko.MpcSetup(model_type=mt, A=ks.model["A"], B=ks.model["B"], m=1, Np=8, projmtx=ks.model["C"][:1], cost_running=1.0,
                    cost_terminal=10.0, cost_input=np.array([0.01]),
                    input_bounds=np.stack([(np.array([-1.0]) - sc["u_offset"]) / sc["u_factor"],
                                           (np.array([1.0]) - sc["u_offset"]) / sc["u_factor"]], axis=1),
                    slope_lim=0.5 * float(np.mean(sc["u_factor"])), smooth_lim=None,
                    state_bounds=(sb - sc["y_offset"][:, None]) / sc["y_factor"][:, None], n=2)
    assert np.abs(s.state_bounds - sb_sc).max() < 1e-12
    oest = ko.estimate_load_linear if mt == "linear" else ko.estimate_load_bilinear
    ref = np.full((9, 1), 0.3)
    v = ks.valdata[0]
    # current states (scaled) inside the bounds; the observation windows from the validation trial
    for t, y_now in ((30, [0.0, 0.0]), (60, [0.05, -0.1]), (90, [-0.1, 0.2])):
        traj = {"y": np.array([y_now]), "u": np.zeros((1, 1))}
        yp, up = v["y"][t - 10:t + 1], v["u"][t - 10:t + 1]
        zeta = traj["y"][0]
        for iters in ((1, 2, 3) if mt == "bilinear" else (1,)):
            U, z, what = mpc.get_mpcInput_loaded(traj, ref, yp, up, iters=iters)
            owhat, _ = oest(dic, ks.model, yp, up, nw, 0, None)
            assert np.abs(what - owhat).max() <= 1e-8
            zo = ko.loaded_lift(ko.econ_full(dic, zeta[None, :]), what[None, :])[0]
            assert np.abs(z - zo).max() <= 1e-13
            Uo, _ = ko.mpc_step(s, zo, traj["u"][-1], ref, iters)
            assert np.isfinite(Uo).all() and np.abs(U - Uo).max() <= 1e-8, (t, iters, np.abs(U - Uo).max())
            Uh, st = mpc.dev.step(z, traj["u"][-1], mpc._pad_ref(ref), iters)
            assert st == 0 and np.abs(U - Uh).max() <= 1e-10
        # a failed estimate (|what_prev| > 1.01 with the rate rows) fails the state-bound step: NaN and KP_ERR_QP_FAIL
        _, zwin = ks.get_zeta({"y": yp, "u": up})
        uwin = up[:10]
        Uf, zf, wf, rnf, stf = mpc.dev.step_loaded(ks.basis_dev, nw, zwin, uwin, np.full(nw, 1.5), mpc.dev.LOAD_RATE, zeta,
                                                   traj["u"][-1], mpc._pad_ref(ref), 2 if mt == "bilinear" else 1)
        assert stf == -4 and np.isnan(Uf).all() and np.isnan(wf).all() and np.isnan(rnf)


def test_fused_loaded_step_refusals(ctx):
    ks, mpc, dic, s = loaded_model("bilinear", 2, 0)
    b, dev = ks.basis_dev, mpc.dev
    v = ks.valdata[0]
    zw, uw = v["y"][:11], v["u"][:10]
    Yr = np.zeros(9)
    with pytest.raises(F.KoopmanHipError, match="nw = 9"):
        dev.step_loaded(b, 9, zw, uw, None, 0, v["y"][0], v["u"][0], Yr)
    with pytest.raises(F.KoopmanHipError, match="nobs = 65"):
        dev.step_loaded(b, 2, v["y"][:66], v["u"][:65], None, 0, v["y"][0], v["u"][0], Yr)
    with pytest.raises(F.KoopmanHipError, match="width"):
        dev.step_loaded(b, 1, zw, uw, None, 0, v["y"][0], v["u"][0], Yr)
    with pytest.raises(F.KoopmanHipError, match="what_prev"):
        dev.step_loaded(b, 2, zw, uw, None, dev.LOAD_RATE, v["y"][0], v["u"][0], Yr)
    # a window beyond the LDS budget: 64 samples of a 457-column dictionary
    big = kra.Basis(ctx, "linear", 5, 1, [("poly", kra.poly_exponent_table(5, 6)[5:])])
    NL = big.N * 2
    rng = np.random.default_rng(0)
    mbig = kra.Mpc(ctx, "linear", 0.5 * np.eye(NL) + 1e-3 * rng.standard_normal((NL, NL)), np.zeros((NL, 1)), 4, np.eye(1, NL), 1.0, 1.0,
                   np.array([0.1]))
    with pytest.raises(F.KoopmanHipError, match="LDS"):
        mbig.step_loaded(big, 1, rng.uniform(-1, 1, (65, 5)), np.zeros((64, 1)), None, 0, np.zeros(5), np.zeros(1), np.zeros(5))
    U, z, what, rn, st = mbig.step_loaded(big, 1, rng.uniform(-1, 1, (3, 5)), np.zeros((2, 1)), None, 0, np.zeros(5), np.zeros(1),
                                          np.zeros(5))
    assert st == 0 and np.isfinite(U).all() and z.shape == (NL,)
    # the estimate's QP infeasible (|what_prev| > 1.01 with the rate rows): NaN and a failed status, never a wrong result
    U, z, what, rn, st = dev.step_loaded(b, 2, zw, uw, np.full(2, 1.5), dev.LOAD_RATE, v["y"][0], v["u"][0], Yr)
    assert st == -4                                                        # KP_ERR_QP_FAIL
    assert np.isnan(U).all() and np.isnan(what).all() and np.isnan(rn)
    mbig.close(); big.close()


def _desc(model_type, nzeta, m, deg):
    e = kra.poly_exponent_table(nzeta, deg)[nzeta:].astype(np.uint8)
    return dict(model_type=np.int32(F.MODEL[model_type]), nzeta=np.int32(nzeta), m=np.int32(m),
                block_type=np.array([[0]], dtype=np.int32), block_count=np.array([[e.shape[0]]], dtype=np.int32),
                poly_exps=np.asfortranarray(e.T), gauss_centres=None, pcs=None), e


def test_loaded_step_through_the_gateway(ctx):
    """[U, z, what, resnorm] = kp_mex('mpc_step', m, zeta, u_prev, Yr, iters, b, nw, Zwin, Uwin, what_prev, flags) equals
    the direct call; size errors are kp:size."""
    import mexshim as ms
    ms.build()
    d, e = _desc("bilinear", 3, 2, 2)
    bp = kra.Basis(ctx, "bilinear", 3, 2, [("poly", e)])
    nw, N = 2, bp.N
    NL = N * (nw + 1)
    rng = np.random.default_rng(4)
    A = np.asfortranarray(0.2 * rng.standard_normal((NL, NL)) / np.sqrt(NL) + 0.5 * np.eye(NL))
    B = np.asfortranarray(0.1 * rng.standard_normal((NL, NL * 2)) / np.sqrt(NL))
    proj = np.hstack([np.eye(2), np.zeros((2, NL - 2))])
    args = (6, proj, 10.0, 100.0, np.array([3e-3, 2e-3]), np.array([-0.9, -0.9]), np.array([0.9, 0.9]), 0.2, None)
    mp = kra.Mpc(ctx, "bilinear", A, B, *args)
    h = ms.kp_mex("create", 0)
    m_ = ms.kp_mex("mpc_create", h, 1, A, B, *args)
    b = ms.kp_mex("basis_create", h, d)
    zw = rng.uniform(-0.5, 0.5, (12, 3)); uw = rng.uniform(-0.3, 0.3, (11, 2))
    zeta = zw[-1]; up = uw[-1]; Yr = rng.uniform(-0.5, 0.5, 2 * 7)
    for wp, flags in ((np.array([]), 0), (np.array([0.1, -0.2]), 1), (np.array([0.1, -0.2]), 3)):
        U, z, what, rn = ms.kp_mex("mpc_step", m_, zeta, up, Yr, 1, b, nw, zw.T, uw.T, wp, flags, nargout=4)
        Ud, zd, wd, rnd, st = mp.step_loaded(bp, nw, zw, uw, wp if wp.size else None, flags, zeta, up, Yr, 1)
        assert st == 0 and np.abs(U - Ud).max() <= 1e-10 and np.abs(z.ravel() - zd).max() <= 1e-14
        assert np.abs(what.ravel() - wd).max() <= 1e-14 and abs(float(np.ravel(rn)[0]) - rnd) <= 1e-14 * max(rnd, 1e-300)
    # no estimate: empty window, the lift with what_prev
    U, z, what = ms.kp_mex("mpc_step", m_, zeta, up, Yr, 1, b, nw, np.zeros((0, 0)), np.zeros((0, 0)), np.array([0.3, 0.1]), 0, nargout=3)
    assert np.array_equal(what.ravel(), [0.3, 0.1]) and np.abs(z.ravel()[N:2 * N] - 0.3 * z.ravel()[:N]).max() <= 1e-15
    for bad in ((zw[:, :2].T, uw.T, np.array([])), (zw.T, uw[:5].T, np.array([])), (zw.T, uw.T, np.array([0.1]))):
        with pytest.raises(ms.MexError) as ei:
            ms.kp_mex("mpc_step", m_, zeta, up, Yr, 1, b, nw, *bad, 0)
        assert ei.value.identifier == "kp:size"
    with pytest.raises(ms.MexError) as ei:
        ms.kp_mex("mpc_step", m_, zeta, up, Yr, 1, b, nw)
    assert ei.value.identifier == "kp:usage"
    with pytest.raises(ms.MexError) as ei:                             # the unloaded form keeps its two outputs
        ms.kp_mex("mpc_step", m_, z.ravel(), up, Yr, nargout=3)
    assert ei.value.identifier == "kp:usage"
    ms.kp_mex("basis_destroy", b, nargout=0)
    ms.kp_mex("mpc_destroy", m_, nargout=0)
    ms.kp_mex("destroy", h, nargout=0)
    mp.close(); bp.close()


def test_stored_circle_runs_run_free_under_plant_load(ctx, golden):
    """The three MATLAB circle runs res{1..3} (the unloaded N = 34 bilinear controller on the arm carrying loads W) run
    free through the product path: device fit, the controller of test_stored_circle_runs_replayed_on_device (slope 1e-2,
    no box), Ksim(Arm, mpc).run_trial_mpc(R(2:end), X(1), U(1), load_value = W).  The reference is R(2:end), so the
    windows after step 289 are padded by repetition while MATLAB saw the longer original: outputs are compared over steps
    0-290, mean tracking errors over the first 290 steps.  res{3} is sensitive past step 200 (an oracle loop leaves the
    stored run there too): its outputs are compared over the first 200 steps.
    Bounds are about 2x those of the same loop run on the CPU with the oracle (ko.mpc_step on the oracle's model,
    Arm.simulate_Ts under W): max |dY| 8.6e-5, 6.2e-4, 1.4e-4 (200 steps) and mean errors 0.1341088, 0.039146, 0.18970
    against the stored 0.1341104, 0.039152, 0.18989.  res{2}'s mean-error bound is 3e-4 relative, not 1e-4: the oracle
    loop itself is 1.5e-4 from the stored run there.  The device loop is also held to the oracle loop's mean errors."""
    g = golden["arm_data"]; c = golden["arm_circle"]; gp = golden["arm_plant"]
    cx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "arm_circle_x.npz"))
    lens = g["train_len"]; off = np.concatenate([[0], np.cumsum(lens)])
    train = [{"t": g["train_t"][a:b], "y": g["train_y"][a:b], "u": g["train_u"][a:b]} for a, b in zip(off[:-1], off[1:])]
    val = [{"t": g["val_t"], "y": g["val_y"], "u": g["val_u"]}]
    ks = kra.Ksysid({"train": train, "val": val}, ctx=ctx, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    snapshots=np.inf, lasso=[np.inf], delays=0, dim_red=True).train_models()
    mpc = kra.Kmpc(ks, horizon=10, input_bounds=[], input_slopeConst=1e-2, input_smoothConst=None, state_bounds=[],
                   cost_running=10, cost_terminal=100, cost_input=0.1 * np.array([3e-2, 2e-2, 1e-2]), projmtx=ks.model["C"][-2:, :])
    params = {k[2:]: (float(gp[k]) if gp[k].ndim == 0 else gp[k]) for k in gp.files if k.startswith("p_")}
    sim = kra.Ksim(kra.Arm(params, output_type="markers"), mpc)
    # steps compared, Y, relative mean error vs the stored run, the oracle loop's mean error and the tolerance against it
    bounds = [(291, 2e-4, 2e-5, 0.1341088, 1e-6), (291, 2e-3, 3e-4, 0.039146, 1e-6), (200, 5e-4, 2e-3, 0.18970, 2e-4)]
    for i, (nk, ytol, etol, omean, otol) in enumerate(bounds):
        X, Y, U, R, W = cx[f"run{i}_X"], c[f"run{i}_Y"], c[f"run{i}_U"], c[f"run{i}_R"], c[f"run{i}_W"]
        assert (W == W[0]).all()
        res = sim.run_trial_mpc(R[1:], X[0], U[0], load_value=W[1:])
        assert res["Y"].shape == (300, 6) and np.array_equal(res["W"], W[1:])
        dy = np.abs(res["Y"][:nk] - Y[:nk]).max()
        stored, mean = float(c[f"run{i}_err"][:290].mean()), float(res["err"][:290].mean())
        rel = abs(mean - stored) / stored
        print(f"res{{{i + 1}}}: max |dY| over {nk} steps {dy:.3e}, mean error {mean:.7f} vs stored {stored:.7f} ({rel:.2e})")
        assert dy <= ytol, (i, dy)
        assert rel <= etol, (i, rel)
        assert abs(mean - omean) <= otol, (i, mean, omean)


class ToyPlant:
    """The loaded system of tests/_loaded_system.py as a Ksim plant."""

    params = {"nx": 2, "nu": 1, "nw": 1}

    def get_y(self, x):
        return np.asarray(x, dtype=np.float64)

    def simulate_Ts(self, x, u, w):
        return toy_step(np.asarray(x, dtype=np.float64), np.ravel(u), np.ravel(w))


def _toy_controller(nd, loaded):
    trials = make_trials(14, 200, nw=1, seed=21)
    if not loaded:
        trials = [{k: v for k, v in t.items() if k != "w"} for t in trials]
    ks = kra.Ksysid({"train": trials[:12], "val": trials[12:]}, model_type="bilinear", obs_type=["poly"], obs_degree=[3],
                    loaded=loaded, delays=nd)
    ks.train_models()
    return kra.Kmpc(ks, horizon=10, input_bounds=[-2.0, 2.0], cost_running=10.0, cost_terminal=100.0, cost_input=0.01,
                    projmtx=ks.model["C"][:2])


@pytest.mark.parametrize("nd", [0, 1])
def test_loaded_closed_loop_end_to_end(nd):
    """A loaded bilinear model of the toy loaded system, its controller in Ksim around the true system under a constant
    load and a step change of load: the fused loop equals the host-assembled one, the estimate settles on the true
    load after the change, and the tracking beats the unloaded controller's on the same loaded plant by at least 5 %.
    Measured mean tracking errors, loaded vs unloaded controller (the loaded one is 12-24 % lower):
      nd = 0: constant load 0.0548 vs 0.0720, step change 0.0518 vs 0.0603;
      nd = 1: constant load 0.0548 vs 0.0647, step change 0.0512 vs 0.0585."""
    t = np.arange(101) * 0.1
    ref = np.column_stack([0.4 * np.sin(t), 0.4 * np.cos(t)])             # a circle in (angle, rate)
    mpc = _toy_controller(nd, True)
    mpc0 = _toy_controller(nd, False)
    sim = kra.Ksim(ToyPlant(), mpc)
    for W in (np.full((101, 1), 0.6), np.vstack([np.full((50, 1), 0.6), np.full((51, 1), -0.5)])):
        mpc.fused_load_step = True
        rf = sim.run_trial_mpc(ref, None, None, load_value=W)
        mpc.fused_load_step = False
        rh = sim.run_trial_mpc(ref, None, None, load_value=W)
        assert rf["Y"].shape == (101, 2) and rh["Y"].shape == (101, 2)
        assert np.abs(rf["Y"] - rh["Y"]).max() <= 1e-9 and np.abs(rf["What"] - rh["What"]).max() <= 1e-9
        assert abs(np.median(rf["What"][70:]) - W[-1, 0]) <= 0.1, rf["What"][70:].ravel()     # 20 steps after the change
        r0 = kra.Ksim(ToyPlant(), mpc0).run_trial_mpc(ref, None, None, load_value=W)
        print(f"nd = {nd}, load {W[0, 0]} -> {W[-1, 0]}: mean tracking error loaded {rf['err'].mean():.5f}, unloaded "
              f"{r0['err'].mean():.5f}, estimate median after step 70 {np.median(rf['What'][70:]):.4f}")
        assert rf["err"].mean() <= 0.95 * r0["err"].mean()
